// rust/shim.rs — the module a SingleRust maintainer adds as `src/gpu/mod.rs` (cargo feature `hip`), next to the
// generated `src/gpu/ffi.rs` (= rust/srx_sys.rs).  It keeps the reference's public signatures and replaces the bodies
// listed in SURVEY.md §8(b) by calls into libsrx_hip.so.  NOT compile-checked: the build image has no rustc / cargo.
// The same call sequences are exercised through ctypes (singlerust_amd/_ffi.py) and through the C++ mirror
// (singlerust_amd/host/single_rust.hpp, tests/cpp/host_mirror_test.cpp), which this file follows function by function.
//
// Replaced bodies (reference file:line):
//   memory::statistics::{compute_number, compute_sum, compute_variance, compute_std_dev, compute_min_max}
//       src/memory/statistics/mod.rs:10-46   -> src/shared/statistics/helper/csr.rs:16-38,81-102,149-228
//   memory::statistics::compute_qc_variables          src/memory/statistics/mod.rs:48-72
//   memory::processing::normalize_total_inplace       src/memory/processing/mod.rs:303-312 -> scale/mod.rs:7-173
//   memory::processing::log1p_transform_inplace       src/memory/processing/mod.rs:324-326 -> transform/mod.rs:36-57
//   memory::processing::dim_red::select_features      src/memory/processing/dim_red/mod.rs:123-156 (HighlyVariable arm)
//   memory::processing::dim_red::pca_inplace          src/memory/processing/dim_red/mod.rs:24-94
//   memory::processing::filter_cells[_inplace] / filter_genes[_inplace]   src/memory/processing/mod.rs:86-146,245-299
//   memory::statistics::qc_vars_inplace               src/memory/statistics/mod.rs:74-103
//   backed::statistics::{compute_number, compute_sum} src/backed/statistics/mod.rs:5-45
mod ffi;                                   // rust/srx_sys.rs
use ffi::*;

use std::ffi::CStr;
use std::ops::Deref;
use std::os::raw::c_void;
use std::ptr::{null, null_mut};

use anndata::data::{ArrayData, DynCscMatrix, DynCsrMatrix};
use anndata_memory::IMAnnData;
use anyhow::{anyhow, bail, Result};

use crate::shared::{Direction, FeatureSelection, FlexValue};

// ---- handles --------------------------------------------------------------------------------------------------
/// One GPU + stream (+ optional communicator).  Not `Sync`: one context per thread, as include/srx.h requires.
pub struct Ctx(*mut SrxCtx);

impl Ctx {
    pub fn new(device_id: i32) -> Result<Self> {
        let mut p = null_mut();
        let rc = unsafe { srx_ctx_create(device_id, &mut p) };
        if rc != SRX_OK {
            return Err(anyhow!(last_error(null())));        // "no HIP device" when the library cannot see a GPU: no CPU fallback
        }
        Ok(Ctx(p))
    }
    fn check(&self, rc: i32) -> Result<()> {
        if rc == SRX_OK { Ok(()) } else { Err(anyhow!(last_error(self.0))) }
    }
}
impl Drop for Ctx {
    fn drop(&mut self) { unsafe { srx_ctx_destroy(self.0) } }
}

fn last_error(ctx: *const SrxCtx) -> String {
    unsafe { CStr::from_ptr(srx_last_error(ctx)) }.to_string_lossy().into_owned()
}

/// Gene lists as the C ABI takes them: (ptr with lists.len() + 1 entries, the genes of every list one after another; never empty).
fn pack_lists(lists: &[Vec<u64>]) -> (Vec<u64>, Vec<u64>) {
    let mut ptr = vec![0u64; lists.len() + 1];
    for (t, l) in lists.iter().enumerate() { ptr[t + 1] = ptr[t] + l.len() as u64; }
    let mut flat: Vec<u64> = lists.iter().flatten().copied().collect();
    if flat.is_empty() { flat.push(0); }
    (ptr, flat)
}

/// Device-resident X of one IMAnnData.  Upload once; every call of the path then works on the handle.
pub struct DeviceX<'c> { ctx: &'c Ctx, mat: *mut SrxMat, n_obs: usize, n_vars: usize }

impl Drop for DeviceX<'_> {
    fn drop(&mut self) { unsafe { srx_matrix_free(self.mat) } }
}

macro_rules! csr_descriptor {
    ($m:expr, $code:expr) => {
        SrxCsr {
            n_rows: $m.nrows() as u64, n_cols: $m.ncols() as u64, nnz: $m.nnz() as u64,
            indptr: $m.row_offsets().as_ptr() as *const u64,       // usize == u64 on x86-64
            indices: $m.col_indices().as_ptr() as *const u64,
            values: $m.values().as_ptr() as *mut c_void,
            dtype: $code,
        }
    };
}
macro_rules! csc_descriptor {
    ($m:expr, $code:expr) => {
        SrxCsr {
            n_rows: $m.nrows() as u64, n_cols: $m.ncols() as u64, nnz: $m.nnz() as u64,
            indptr: $m.col_offsets().as_ptr() as *const u64,
            indices: $m.row_indices().as_ptr() as *const u64,
            values: $m.values().as_ptr() as *mut c_void,
            dtype: $code,
        }
    };
}

/// What `DeviceX::highly_variable_genes_seurat_v3` returns: the selection in rank order and the per-gene columns under scanpy's
/// names (`highly_variable_rank` is NaN where no batch ranks the gene within `n_top_genes`).
pub struct SeuratV3Hvg {
    pub selected: Vec<u64>,
    pub means: Vec<f64>,
    pub variances: Vec<f64>,
    pub variances_norm: Vec<f64>,
    pub highly_variable_rank: Vec<f64>,
    pub highly_variable_nbatches: Vec<u32>,
    pub info: SrxSeuratV3Info,
}

impl<'c> DeviceX<'c> {
    /// Takes the same read guard the reference takes (statistics/mod.rs:11-13) for the duration of the copy.
    pub fn upload(ctx: &'c Ctx, adata: &IMAnnData) -> Result<Self> {
        let x = adata.x();
        let guard = x.0.read_inner();
        let mut mat = null_mut();
        macro_rules! up { ($d:expr, $f:ident) => {{ let h = $d; ctx.check(unsafe { $f(ctx.0, &h, SRX_STORE_AUTO, &mut mat) })?; }}; }
        match guard.deref() {
            // dtype set of match_dyn_csr_matrix! (src/shared/mod.rs:110-129); anything else stays the reference's panic
            ArrayData::CsrMatrix(d) => match d {
                DynCsrMatrix::I8(m) => up!(csr_descriptor!(m, SRX_I8), srx_matrix_upload),
                DynCsrMatrix::I16(m) => up!(csr_descriptor!(m, SRX_I16), srx_matrix_upload),
                DynCsrMatrix::I32(m) => up!(csr_descriptor!(m, SRX_I32), srx_matrix_upload),
                DynCsrMatrix::U8(m) => up!(csr_descriptor!(m, SRX_U8), srx_matrix_upload),
                DynCsrMatrix::U16(m) => up!(csr_descriptor!(m, SRX_U16), srx_matrix_upload),
                DynCsrMatrix::U32(m) => up!(csr_descriptor!(m, SRX_U32), srx_matrix_upload),
                DynCsrMatrix::F32(m) => up!(csr_descriptor!(m, SRX_F32), srx_matrix_upload),
                DynCsrMatrix::F64(m) => up!(csr_descriptor!(m, SRX_F64), srx_matrix_upload),
                _ => panic!("CSR matrices of this dtype are not supported for this operation"),
            },
            ArrayData::CscMatrix(d) => match d {
                DynCscMatrix::I8(m) => up!(csc_descriptor!(m, SRX_I8), srx_matrix_upload_csc),
                DynCscMatrix::I16(m) => up!(csc_descriptor!(m, SRX_I16), srx_matrix_upload_csc),
                DynCscMatrix::I32(m) => up!(csc_descriptor!(m, SRX_I32), srx_matrix_upload_csc),
                DynCscMatrix::U8(m) => up!(csc_descriptor!(m, SRX_U8), srx_matrix_upload_csc),
                DynCscMatrix::U16(m) => up!(csc_descriptor!(m, SRX_U16), srx_matrix_upload_csc),
                DynCscMatrix::U32(m) => up!(csc_descriptor!(m, SRX_U32), srx_matrix_upload_csc),
                DynCscMatrix::F32(m) => up!(csc_descriptor!(m, SRX_F32), srx_matrix_upload_csc),
                DynCscMatrix::F64(m) => up!(csc_descriptor!(m, SRX_F64), srx_matrix_upload_csc),
                _ => panic!("CSC matrices of this dtype are not supported for this operation"),
            },
            _ => bail!("X is neither a CSC nor a CSR matrix"),
        }
        Ok(DeviceX { ctx, mat, n_obs: adata.n_obs(), n_vars: adata.n_vars() })
    }
    fn len(&self, d: &Direction) -> usize { if d.is_row() { self.n_obs } else { self.n_vars } }
    fn dir(d: &Direction) -> i32 { if d.is_row() { SRX_ROW } else { SRX_COLUMN } }

    // ---- memory::statistics ----------------------------------------------------------------------------------
    pub fn compute_number(&self, direction: Direction) -> Result<Vec<u32>> {
        let mut v = vec![0u32; self.len(&direction)];
        self.ctx.check(unsafe { srx_compute_number(self.mat, Self::dir(&direction), v.as_mut_ptr()) })?;
        Ok(v)
    }
    pub fn compute_sum(&self, direction: Direction) -> Result<Vec<f64>> {
        let mut v = vec![0f64; self.len(&direction)];
        self.ctx.check(unsafe { srx_compute_sum(self.mat, Self::dir(&direction), v.as_mut_ptr()) })?;
        Ok(v)
    }
    pub fn compute_variance(&self, direction: Direction) -> Result<Vec<f64>> {
        let mut v = vec![0f64; self.len(&direction)];
        self.ctx.check(unsafe { srx_compute_variance(self.mat, Self::dir(&direction), v.as_mut_ptr()) })?;
        Ok(v)
    }
    pub fn compute_std_dev(&self, direction: Direction) -> Result<Vec<f64>> {
        let mut v = vec![0f64; self.len(&direction)];
        self.ctx.check(unsafe { srx_compute_std_dev(self.mat, Self::dir(&direction), v.as_mut_ptr()) })?;
        Ok(v)
    }
    pub fn compute_min_max(&self, direction: Direction) -> Result<(Vec<f64>, Vec<f64>)> {
        let n = self.len(&direction);
        let (mut mn, mut mx) = (vec![0f64; n], vec![0f64; n]);
        self.ctx.check(unsafe { srx_compute_min_max(self.mat, Self::dir(&direction), mn.as_mut_ptr(), mx.as_mut_ptr()) })?;
        Ok((mn, mx))
    }
    /// The eight vectors of `StatisticsContainer` (statistics/mod.rs:48-72) from one row pass + one column pass.
    #[allow(clippy::type_complexity)]
    pub fn compute_qc_variables(&self) -> Result<(Vec<u32>, Vec<u32>, Vec<f64>, Vec<f64>, Vec<f64>, Vec<f64>, Vec<f64>, Vec<f64>)> {
        let (c, g) = (self.n_obs, self.n_vars);
        let (mut num_cell, mut num_gene) = (vec![0u32; c], vec![0u32; g]);
        let (mut expr_gene, mut expr_cell) = (vec![0f64; g], vec![0f64; c]);
        let (mut var_gene, mut var_cell, mut sd_cell, mut sd_gene) = (vec![0f64; g], vec![0f64; c], vec![0f64; c], vec![0f64; g]);
        self.ctx.check(unsafe {
            srx_compute_qc_variables(self.mat, num_cell.as_mut_ptr(), num_gene.as_mut_ptr(), expr_gene.as_mut_ptr(),
                                     expr_cell.as_mut_ptr(), var_gene.as_mut_ptr(), var_cell.as_mut_ptr(),
                                     sd_cell.as_mut_ptr(), sd_gene.as_mut_ptr())
        })?;
        Ok((num_cell, num_gene, expr_gene, expr_cell, var_gene, var_cell, sd_cell, sd_gene))
    }

    // ---- memory::processing ----------------------------------------------------------------------------------
    /// scale/mod.rs:7-23: `scale = if sum == 0 { 0 } else { target / sum }`, `v * scale`; the logical dtype becomes F64.
    pub fn normalize_total_inplace(&mut self, target_sum: f64, direction: Direction) -> Result<()> {
        self.ctx.check(unsafe { srx_normalize_total_inplace(self.mat, target_sum, Self::dir(&direction)) })
    }
    /// transform/mod.rs:36-57: F32 stays F32, everything else becomes F64.
    pub fn log1p_transform_inplace(&mut self) -> Result<()> {
        self.ctx.check(unsafe { srx_log1p_inplace(self.mat) })
    }
    /// Values back into a host `Vec<f64>` for `*csr_matrix = DynCsrMatrix::F64(..)` (scale/mod.rs:82) — only when the
    /// host copy is needed; the pipeline itself never leaves the device.
    pub fn download_values_f64(&self, nnz: usize) -> Result<Vec<f64>> {
        let mut v = vec![0f64; nnz];
        self.ctx.check(unsafe { srx_matrix_download_values(self.mat, v.as_mut_ptr() as *mut c_void, SRX_F64) })?;
        Ok(v)
    }

    fn flex(v: &FlexValue) -> SrxFlex {          // src/shared/mod.rs:62-66
        match v {
            FlexValue::Absolute(a) => SrxFlex { kind: SRX_FLEX_ABSOLUTE, absolute: *a, relative: 0.0 },
            FlexValue::Relative(p) => SrxFlex { kind: SRX_FLEX_RELATIVE, absolute: 0, relative: *p },
            FlexValue::None => SrxFlex { kind: SRX_FLEX_NONE, absolute: 0, relative: 0.0 },
        }
    }
    /// processing/mod.rs:86-146: returns the filtered matrix and the keep-mask that drives the `obs` subset.
    pub fn filter_cells(&self, lower: &FlexValue, upper: &FlexValue) -> Result<(DeviceX<'c>, Vec<bool>)> {
        let mut out = null_mut();
        let mut mask = vec![0u8; self.n_obs];
        self.ctx.check(unsafe { srx_filter_cells(self.mat, Self::flex(lower), Self::flex(upper), &mut out, mask.as_mut_ptr()) })?;
        let keep: Vec<bool> = mask.iter().map(|&b| b != 0).collect();
        let n_obs = keep.iter().filter(|&&k| k).count();
        Ok((DeviceX { ctx: self.ctx, mat: out, n_obs, n_vars: self.n_vars }, keep))
    }
    /// processing/mod.rs:245-299.
    pub fn filter_genes(&self, lower: &FlexValue, upper: &FlexValue) -> Result<(DeviceX<'c>, Vec<bool>)> {
        let mut out = null_mut();
        let mut mask = vec![0u8; self.n_vars];
        self.ctx.check(unsafe { srx_filter_genes(self.mat, Self::flex(lower), Self::flex(upper), &mut out, mask.as_mut_ptr()) })?;
        let keep: Vec<bool> = mask.iter().map(|&b| b != 0).collect();
        let n_vars = keep.iter().filter(|&&k| k).count();
        Ok((DeviceX { ctx: self.ctx, mat: out, n_obs: self.n_obs, n_vars }, keep))
    }

    // ---- memory::processing::dim_red ---------------------------------------------------------------------------
    /// dim_red/mod.rs:123-156.  `HighlyVariable(n)`: stable descending sort of the non-zero-only gene variance, the
    /// first n indices in rank order (:135-140) — computed on the device; the other arms are host-side index lists.
    pub fn select_features(&self, fs: &FeatureSelection) -> Result<Option<Vec<u64>>> {
        match fs {
            FeatureSelection::HighlyVariable(n) => {
                let mut idx = vec![0u64; (*n).min(self.n_vars)];
                let mut n_out = 0u64;
                self.ctx.check(unsafe { srx_select_hvg(self.mat, *n as u64, idx.as_mut_ptr(), &mut n_out) })?;
                idx.truncate(n_out as usize);
                Ok(Some(idx))
            }
            FeatureSelection::None => Ok(None),      // all genes: `sel = NULL`
            // HighlyVariableCol / Randomized / VarianceThreshold keep the reference's host code (:125-134,141-153): it
            // builds the index list from a var column, an RNG or `compute_variance` (replaced above); hand that list
            // to `pca_with_selection`
            _ => bail!("feature selection arm handled on the host: pass its index list to pca_with_selection"),
        }
    }

    /// Not in the reference: scanpy's `highly_variable_genes(flavor = "pearson_residuals")` on the RAW counts (srx.h states the
    /// definition).  Returns (the selected genes in rank order, the residual variance of every gene, the info block); `theta`
    /// `None` = 100, `clip` `None` = sqrt(n_obs).  Hand the list to `pca_with_selection` after normalize / log1p.
    pub fn highly_variable_genes_pearson(&self, n_top_genes: usize, theta: Option<f64>, clip: Option<f64>)
                                         -> Result<(Vec<u64>, Vec<f64>, SrxPearsonInfo)> {
        let opts = SrxPearsonOpts { theta: theta.unwrap_or(0.0), clip: clip.unwrap_or(0.0) };
        let mut idx = vec![0u64; n_top_genes.min(self.n_vars).max(1)];
        let mut var = vec![0f64; self.n_vars.max(1)];
        let mut n_out = 0u64;
        let mut info: SrxPearsonInfo = unsafe { std::mem::zeroed() };
        self.ctx.check(unsafe {
            srx_select_hvg_pearson(self.mat, n_top_genes as u64, &opts, idx.as_mut_ptr(), &mut n_out, var.as_mut_ptr(), &mut info)
        })?;
        idx.truncate(n_out as usize);
        var.truncate(self.n_vars);
        Ok((idx, var, info))
    }

    /// Not in the reference: scanpy's `highly_variable_genes(flavor = "seurat_v3", batch_key = ..)` on the RAW counts (srx.h
    /// states the definition: a direct loess surface).  `batch`: one code below `n_batches` per cell, `None` = one batch;
    /// `span` `None` = 0.3; `paper_order`: the order of "seurat_v3_paper".  Returns the selected genes in rank order and the
    /// per-gene columns under scanpy's names.
    pub fn highly_variable_genes_seurat_v3(&self, n_top_genes: usize, batch: Option<&[u32]>, n_batches: u32, span: Option<f64>,
                                           paper_order: bool) -> Result<SeuratV3Hvg> {
        if let Some(b) = batch {
            if b.len() != self.n_obs { bail!("highly_variable_genes_seurat_v3: {} batch labels for {} cells", b.len(), self.n_obs); }
        }
        let opts = SrxSeuratV3Opts { span: span.unwrap_or(0.0), paper_order: paper_order as i32, reserved: 0 };
        let g = self.n_vars.max(1);
        let mut r = SeuratV3Hvg { selected: vec![0u64; n_top_genes.min(self.n_vars).max(1)], means: vec![0f64; g], variances: vec![0f64; g],
                                  variances_norm: vec![0f64; g], highly_variable_rank: vec![0f64; g],
                                  highly_variable_nbatches: vec![0u32; g], info: unsafe { std::mem::zeroed() } };
        let mut t: SrxSeuratV3Tables = unsafe { std::mem::zeroed() };
        t.means = r.means.as_mut_ptr();
        t.variances = r.variances.as_mut_ptr();
        t.variances_norm = r.variances_norm.as_mut_ptr();
        t.median = r.highly_variable_rank.as_mut_ptr();
        t.nbatches = r.highly_variable_nbatches.as_mut_ptr();
        let mut n_out = 0u64;
        self.ctx.check(unsafe {
            srx_select_hvg_seurat_v3(self.mat, n_top_genes as u64, batch.map_or(std::ptr::null(), |b| b.as_ptr()),
                                     if batch.is_some() { n_batches } else { 1 }, &opts, r.selected.as_mut_ptr(), &mut n_out, &mut t,
                                     &mut r.info)
        })?;
        r.selected.truncate(n_out as usize);
        for v in [&mut r.means, &mut r.variances, &mut r.variances_norm, &mut r.highly_variable_rank] { v.truncate(self.n_vars); }
        r.highly_variable_nbatches.truncate(self.n_vars);
        Ok(r)
    }

    /// scanpy's `normalize_pearson_residuals` restricted to a gene list: n_obs x genes.len() clipped residuals, row-major,
    /// zeros included; genes in any order, repeats allowed.
    pub fn pearson_residuals(&self, genes: &[u64], theta: Option<f64>, clip: Option<f64>) -> Result<Vec<f64>> {
        let opts = SrxPearsonOpts { theta: theta.unwrap_or(0.0), clip: clip.unwrap_or(0.0) };
        let mut out = vec![0f64; (self.n_obs * genes.len()).max(1)];
        self.ctx.check(unsafe {
            srx_pearson_residuals(self.mat, genes.as_ptr(), genes.len() as u64, &opts, out.as_mut_ptr(), null_mut())
        })?;
        out.truncate(self.n_obs * genes.len());
        Ok(out)
    }

    /// scanpy's `normalize_pearson_residuals_pca` on the RAW counts: PCA of the clipped residuals of `genes` (srx.h states the
    /// definition).  Returns (scores n_obs x n_pc row-major, components genes.len() x n_pc, explained variance ratio, the info
    /// block); the scores also stay resident as the handle's PCA result.  `selected_totals`: the cell sums and the total over
    /// the listed genes (scanpy) instead of the whole matrix.
    pub fn pca_pearson_residuals(&self, genes: &[u64], n_components: usize, theta: Option<f64>, clip: Option<f64>,
                                 selected_totals: bool, center: bool) -> Result<(Vec<f64>, Vec<f64>, Vec<f64>, SrxPearsonPcaInfo)> {
        let mut opts: SrxPearsonPcaOpts = unsafe { std::mem::zeroed() };
        opts.pearson = SrxPearsonOpts { theta: theta.unwrap_or(0.0), clip: clip.unwrap_or(0.0) };
        opts.totals = if selected_totals { 1 } else { 0 };
        opts.center = if center { 1 } else { 0 };
        opts.pca.n_components = n_components as i32;
        opts.pca.center = -1;
        let n_pc = n_components.min(genes.len());
        let mut scores = vec![0f64; (self.n_obs * n_pc).max(1)];
        let mut comps = vec![0f64; (genes.len() * n_pc).max(1)];
        let mut evr = vec![0f64; n_pc.max(1)];
        let mut info: SrxPearsonPcaInfo = unsafe { std::mem::zeroed() };
        self.ctx.check(unsafe {
            srx_pca_pearson(self.mat, genes.as_ptr(), genes.len() as u64, &opts, scores.as_mut_ptr(), comps.as_mut_ptr(),
                            evr.as_mut_ptr(), null_mut(), &mut info)
        })?;
        scores.truncate(self.n_obs * n_pc);
        comps.truncate(genes.len() * n_pc);
        evr.truncate(n_pc);
        Ok((scores, comps, evr, info))
    }

    /// scanpy's `regress_out` -> `scale(max_value)` -> `pca` on the values as stored: `covariates` (n_obs x n_cov row-major; empty:
    /// plain scale + clip) regressed out of `genes`, the residuals scaled and clipped (`max_value` None: no clip), then their PCA
    /// (srx.h states the definition).  Returns (scores, components, explained variance ratio, the info block); the scores also
    /// stay resident as the handle's PCA result.
    pub fn pca_regress_scale(&self, genes: &[u64], covariates: &[f64], n_cov: usize, n_components: usize, scale: bool,
                             max_value: Option<f64>) -> Result<(Vec<f64>, Vec<f64>, Vec<f64>, SrxRegressInfo)> {
        assert_eq!(covariates.len(), self.n_obs * n_cov);
        let mut opts: SrxRegressOpts = unsafe { std::mem::zeroed() };
        opts.scale = if scale { 1 } else { 0 };
        opts.max_value = max_value.unwrap_or(0.0);
        opts.pca.n_components = n_components as i32;
        opts.pca.center = -1;
        let n_pc = n_components.min(genes.len());
        let mut scores = vec![0f64; (self.n_obs * n_pc).max(1)];
        let mut comps = vec![0f64; (genes.len() * n_pc).max(1)];
        let mut evr = vec![0f64; n_pc.max(1)];
        let mut info: SrxRegressInfo = unsafe { std::mem::zeroed() };
        let cov = if n_cov > 0 { covariates.as_ptr() } else { std::ptr::null() };
        self.ctx.check(unsafe {
            srx_pca_regress(self.mat, genes.as_ptr(), genes.len() as u64, cov, n_cov as u64, &opts, scores.as_mut_ptr(),
                            comps.as_mut_ptr(), evr.as_mut_ptr(), null_mut(), null_mut(), &mut info)
        })?;
        scores.truncate(self.n_obs * n_pc);
        comps.truncate(genes.len() * n_pc);
        evr.truncate(n_pc);
        Ok((scores, comps, evr, info))
    }

    /// The regressed, scaled and clipped values of `genes` (n_obs x genes.len() row-major): `srx_regress_residuals`.
    pub fn regress_out(&self, genes: &[u64], covariates: &[f64], n_cov: usize, scale: bool, max_value: Option<f64>) -> Result<Vec<f64>> {
        assert_eq!(covariates.len(), self.n_obs * n_cov);
        let mut opts: SrxRegressOpts = unsafe { std::mem::zeroed() };
        opts.scale = if scale { 1 } else { 0 };
        opts.max_value = max_value.unwrap_or(0.0);
        let mut out = vec![0f64; (self.n_obs * genes.len()).max(1)];
        let cov = if n_cov > 0 { covariates.as_ptr() } else { std::ptr::null() };
        self.ctx.check(unsafe {
            srx_regress_residuals(self.mat, genes.as_ptr(), genes.len() as u64, cov, n_cov as u64, &opts, out.as_mut_ptr(), null_mut())
        })?;
        out.truncate(self.n_obs * genes.len());
        Ok(out)
    }

    /// Per cell and gene list the sum and the number of the stored entries whose gene is in the list (n_obs x lists.len()
    /// row-major each; a stored 0 counts): `srx_gene_list_sums`, one walk over the column indices per 64 lists.
    pub fn gene_list_sums(&self, lists: &[Vec<u64>]) -> Result<(Vec<f64>, Vec<u32>, SrxGeneListInfo)> {
        let (ptr, flat) = pack_lists(lists);
        let mut sum = vec![0f64; (self.n_obs * lists.len()).max(1)];
        let mut cnt = vec![0u32; (self.n_obs * lists.len()).max(1)];
        let mut info: SrxGeneListInfo = unsafe { std::mem::zeroed() };
        self.ctx.check(unsafe {
            srx_gene_list_sums(self.mat, ptr.as_ptr(), flat.as_ptr(), lists.len() as u64, sum.as_mut_ptr(), cnt.as_mut_ptr(), &mut info)
        })?;
        sum.truncate(self.n_obs * lists.len());
        cnt.truncate(self.n_obs * lists.len());
        Ok((sum, cnt, info))
    }

    /// scanpy's `score_genes` on the values as stored, every set of `sets` in one call: per cell the mean over the set minus
    /// the mean over its control genes (srx.h states the definition; the controls of a bin are chosen by a hash of `seed` and
    /// the gene, not by numpy's generator).  Returns (scores n_obs x sets.len() row-major, the control list of every set, the
    /// info block).  `ctrl_size` 0 = 50, `n_bins` 0 = 25, `gene_pool` None = every gene.
    pub fn score_genes(&self, sets: &[Vec<u64>], ctrl_size: u32, n_bins: u32, gene_pool: Option<&[u64]>, seed: u64,
                       ctrl_as_ref: bool) -> Result<(Vec<f64>, Vec<Vec<u64>>, SrxScoreGenesInfo)> {
        let (ptr, flat) = pack_lists(sets);
        let opts = SrxScoreGenesOpts { ctrl_size, n_bins, seed, ctrl_as_ref: if ctrl_as_ref { 1 } else { 0 }, reserved: 0 };
        let n_pool = gene_pool.map_or(self.n_vars, |p| p.len());
        // the bound of srx.h: per set ctrl_size * min(|set|, P / n_items + 1)
        let size = if ctrl_size == 0 { 50 } else { ctrl_size as usize };
        let bins = if n_bins == 0 { 25 } else { n_bins as usize };
        let n_items = ((n_pool as f64 / (bins.max(2) - 1) as f64).round_ties_even() as usize).max(1);
        let capacity: usize = sets.iter().map(|s| size * s.len().min(n_pool / n_items + 1)).sum::<usize>().max(1);
        let mut score = vec![0f64; (self.n_obs * sets.len()).max(1)];
        let mut ctrl_ptr = vec![0u64; sets.len() + 1];
        let mut ctrl = vec![0u64; capacity];
        let mut info: SrxScoreGenesInfo = unsafe { std::mem::zeroed() };
        let (pool, pool_len) = gene_pool.map_or((std::ptr::null(), 0u64), |p| (p.as_ptr(), p.len() as u64));
        self.ctx.check(unsafe {
            srx_score_genes(self.mat, ptr.as_ptr(), flat.as_ptr(), sets.len() as u64, pool, pool_len, &opts, score.as_mut_ptr(),
                            ctrl_ptr.as_mut_ptr(), ctrl.as_mut_ptr(), capacity as u64, &mut info)
        })?;
        score.truncate(self.n_obs * sets.len());
        let lists = (0..sets.len()).map(|s| ctrl[ctrl_ptr[s] as usize..ctrl_ptr[s + 1] as usize].to_vec()).collect();
        Ok((score, lists, info))
    }

    /// scanpy's `score_genes_cell_cycle`: both sets in one call with `ctrl_size = min(|s|, |g2m|)`, then the phase on the
    /// host — "S" by default, "G2M" where G2M > S, "G1" where both are < 0.  Returns (S_score, G2M_score, phase).
    pub fn score_genes_cell_cycle(&self, s_genes: &[u64], g2m_genes: &[u64]) -> Result<(Vec<f64>, Vec<f64>, Vec<&'static str>)> {
        let ctrl_size = s_genes.len().min(g2m_genes.len()) as u32;
        let (score, _, _) = self.score_genes(&[s_genes.to_vec(), g2m_genes.to_vec()], ctrl_size, 25, None, 0, true)?;
        let s: Vec<f64> = score.iter().step_by(2).copied().collect();
        let g: Vec<f64> = score.iter().skip(1).step_by(2).copied().collect();
        let phase = s.iter().zip(&g).map(|(&s, &g)| if s < 0.0 && g < 0.0 { "G1" } else if g > s { "G2M" } else { "S" }).collect();
        Ok((s, g, phase))
    }

    /// The `qc_vars` part of scanpy's `calculate_qc_metrics`: per subset (total_counts, pct_counts = 100 * total / the cell's
    /// sum with 0 / 0 kept as NaN, n_genes_by_counts = the cell's STORED entries in the subset, an explicit 0 included), each
    /// n_obs x subsets.len() row-major.
    pub fn qc_gene_fractions(&self, subsets: &[Vec<u64>]) -> Result<(Vec<f64>, Vec<f64>, Vec<u32>)> {
        let (sum, cnt, _) = self.gene_list_sums(subsets)?;
        let total = self.compute_sum(Direction::Row)?;
        let pct = sum.iter().enumerate().map(|(e, &s)| 100.0 * s / total[e / subsets.len()]).collect();
        Ok((sum, pct, cnt))
    }

    /// dim_red/mod.rs:24-94 without the dense N x k matrix: returns (scores N x n_pc row-major, explained variance
    /// ratio, selected features) — exactly what `attach_pca_results` (:96-121) takes; `n_threads` is accepted and ignored,
    /// the `svd_mode` marker has no counterpart.
    pub fn pca(&self, n_components: Option<usize>, center: Option<bool>, scale: Option<bool>, _n_threads: Option<usize>,
               feature_selection: &FeatureSelection) -> Result<(Vec<f64>, Vec<f64>, Vec<usize>, usize)> {
        let sel = self.select_features(feature_selection)?;
        self.pca_with_selection(n_components, center, scale, sel)
    }

    /// `sel`: feature indices in selection order (`None` = all genes, FeatureSelection::None).
    pub fn pca_with_selection(&self, n_components: Option<usize>, center: Option<bool>, scale: Option<bool>,
                              sel: Option<Vec<u64>>) -> Result<(Vec<f64>, Vec<f64>, Vec<usize>, usize)> {
        let k = sel.as_ref().map_or(self.n_vars, |s| s.len());
        let n_pc = n_components.unwrap_or(2).min(k);                                      // :52
        let opt = |o: Option<bool>| o.map_or(-1, |b| b as i32);                            // None -> library default (true, :55-56)
        let opts = SrxPcaOpts { n_components: n_pc as i32, center: opt(center), scale: opt(scale), n_threads: -1,
                                block: 0, max_iter: 0, solver: SRX_SOLVER_AUTO, tol: 0.0, seed: 0 };
        let mut scores = vec![0f64; self.n_obs * n_pc];
        let mut evr = vec![0f64; n_pc];
        let mut info: SrxPcaInfo = unsafe { std::mem::zeroed() };
        self.ctx.check(unsafe {
            srx_pca(self.mat, sel.as_ref().map_or(null(), |s| s.as_ptr()), k as u64, &opts, scores.as_mut_ptr(),
                    null_mut(), evr.as_mut_ptr(), null_mut(), null_mut(), &mut info)
        })?;
        let selected: Vec<usize> = sel.map_or_else(|| (0..self.n_vars).collect(), |s| s.into_iter().map(|i| i as usize).collect());
        Ok((scores, evr, selected, n_pc))
    }
}

// ---- the reference's public functions, bodies replaced ----------------------------------------------------------
// (each takes the thread's context; a real integration keeps one `Ctx` + `DeviceX` alive next to the IMAnnData so that
//  the five calls of the canonical pipeline — SURVEY.md §3.6 — share one upload)
pub fn compute_number(ctx: &Ctx, adata: &IMAnnData, direction: Direction) -> Result<Vec<u32>> {
    DeviceX::upload(ctx, adata)?.compute_number(direction)
}
pub fn compute_sum(ctx: &Ctx, adata: &IMAnnData, direction: Direction) -> Result<Vec<f64>> {
    DeviceX::upload(ctx, adata)?.compute_sum(direction)
}
pub fn compute_variance(ctx: &Ctx, adata: &IMAnnData, direction: Direction) -> Result<Vec<f64>> {
    DeviceX::upload(ctx, adata)?.compute_variance(direction)
}
pub fn compute_std_dev(ctx: &Ctx, adata: &IMAnnData, direction: Direction) -> Result<Vec<f64>> {
    DeviceX::upload(ctx, adata)?.compute_std_dev(direction)
}
pub fn compute_min_max(ctx: &Ctx, adata: &IMAnnData, direction: Direction) -> Result<(Vec<f64>, Vec<f64>)> {
    DeviceX::upload(ctx, adata)?.compute_min_max(direction)
}

/// normalize_total_inplace -> log1p_transform_inplace -> pca_inplace(.., HighlyVariable(n_hvg)) in ONE library call with
/// every intermediate in HBM (`srx_pipeline`); scores / ratio come back through `srx_result_fetch`.
pub fn pipeline(ctx: &Ctx, adata: &mut IMAnnData, target_sum: f64, n_hvg: usize, n_components: usize)
                -> Result<(Vec<f64>, Vec<f64>, Vec<usize>)> {
    let x = DeviceX::upload(ctx, adata)?;
    let opts = SrxPcaOpts { n_components: n_components as i32, center: -1, scale: -1, n_threads: -1, block: 0, max_iter: 0,
                            solver: SRX_SOLVER_AUTO, tol: 0.0, seed: 0 };
    let mut res: SrxPipelineResult = unsafe { std::mem::zeroed() };
    ctx.check(unsafe { srx_pipeline(x.mat, target_sum, n_hvg as u64, &opts, &mut res) })?;
    let (k, n_pc) = (res.pca.k as usize, res.pca.n_pc as usize);
    let (mut scores, mut evr, mut hvg) = (vec![0f64; x.n_obs * n_pc], vec![0f64; n_pc], vec![0u64; k]);
    ctx.check(unsafe {
        srx_result_fetch(x.mat, scores.as_mut_ptr(), null_mut(), evr.as_mut_ptr(), null_mut(), null_mut(), hvg.as_mut_ptr())
    })?;
    Ok((scores, evr, hvg.into_iter().map(|i| i as usize).collect()))
}

// ================================================================================================================
// The reference's FREE FUNCTIONS with their exact signatures (no context argument): what `src/memory/statistics/mod.rs`,
// `src/memory/processing/mod.rs` and `src/memory/processing/dim_red/mod.rs` export today, bodies replaced.  A caller of
// SingleRust recompiles against the `hip` feature and changes nothing.  The context lives in a `thread_local!` (one per
// thread, as include/srx.h requires); X is uploaded under the reference's own guard ONCE per matrix (resident-handle cache
// below), every call works on the handle and — for the in-place operations — the result goes back into the IMAnnData,
// INCLUDING the variant change to `DynCsrMatrix::F64` that `scale_row_csr` performs (scale/mod.rs:74-83): at once by
// default, on `flush` under `set_lazy_writeback(true)`.  `pipeline()` above is the one-call form (nothing copied back but
// the scores).
// ================================================================================================================
use std::cell::OnceCell;
use std::ops::DerefMut;

use anndata::data::array::ArrayData as AD;
use anndata_memory::IMArrayElement;
use nalgebra_sparse::{CscMatrix, CsrMatrix};
use ndarray::Array2;
use single_algebra::svd::SVDImplementation;            // the marker trait of pca_inplace's last argument (dim_red/mod.rs:12)

// One thread-local holds BOTH the context and the resident handle: struct fields drop in declaration order, so the resident
// matrix (srx_matrix_free) always goes before its context (srx_ctx_destroy) at thread exit, whichever of flush() /
// invalidate() / a compute call touched the thread-local first.  (Two separate `thread_local!`s are destroyed in reverse
// order of their FIRST USE: a first call to flush() registered RESIDENT before CTX — use after free at thread exit.)
struct Tls {
    resident: RefCell<Option<Resident>>,          // dropped first
    lazy_writeback: Cell<bool>,
    ctx: OnceCell<Ctx>,                           // dropped last
}
thread_local! {
    static TLS: Tls = const { Tls { resident: RefCell::new(None), lazy_writeback: Cell::new(false), ctx: OnceCell::new() } };
}
/// The thread's context: device `SRX_DEVICE` (default 0), created on first use.
fn with_ctx<R>(f: impl FnOnce(&Ctx) -> Result<R>) -> Result<R> {
    TLS.with(|t| {
        if t.ctx.get().is_none() {
            let dev = std::env::var("SRX_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            let _ = t.ctx.set(Ctx::new(dev)?);
        }
        f(t.ctx.get().expect("context"))
    })
}

// ---- resident-handle cache ------------------------------------------------------------------------------------------
// The free functions below keep ONE uploaded X per thread, keyed on the identity of the IMAnnData's X element: the canonical
// sequence normalize_total_inplace -> log1p_transform_inplace -> pca_inplace uploads once.  An in-place
// operation runs on the device and then either copies the values back at once (the default: the IMAnnData is current after
// every call, exactly as with the reference) or, under `set_lazy_writeback(true)`, only marks the host copy stale — `flush`
// (called by every function here that hands X to host code, and by the caller before touching `adata.x()` directly) brings
// it back.  `invalidate()` drops the handle: for callers that modify X behind the shim's back.
use std::cell::{Cell, RefCell};

struct Resident {
    key: XKey,
    _x_elem: IMArrayElement,                    // a clone of the X slot's Arc: while the cache holds it the allocation cannot be
                                                // freed, so its ADDRESS (part of the key) cannot be recycled by another matrix
    dev: DeviceX<'static>,                      // (the context is the thread's own, alive as long as the thread)
    host_stale: bool,                           // the device holds newer values than the IMAnnData
    keep_f32: bool,                             // how the pending write-back treats an F32 matrix (log1p keeps it F32)
}
pub fn set_lazy_writeback(on: bool) { TLS.with(|t| t.lazy_writeback.set(on)) }
/// Drops the resident handle: for callers that modify X behind the shim's back (a host-side edit that keeps the shape, the
/// number of stored entries and the variant is invisible to the key).
pub fn invalidate() { TLS.with(|t| *t.resident.borrow_mut() = None) }

/// Identity of the X element: the address of the slot's shared allocation (`IMArrayElement(Slot<ArrayData>)`, an
/// `Arc<RwLock<..>>` — a deep clone has its own; the cache keeps a clone of the Arc, so the address stays taken) together
/// with the shape, the number of stored entries and the VARIANT (storage format + dtype: normalize_total on a host copy
/// changes it, scale/mod.rs:82).
type XKey = (usize, usize, usize, usize, u32);
fn x_key(adata: &IMAnnData) -> XKey {
    let x = adata.x();
    let (nnz, variant) = match x.0.read_inner().deref() {
        ArrayData::CsrMatrix(m) => (m.nnz(), 0x100 | dyn_csr_dtype(m)),
        ArrayData::CscMatrix(m) => (m.nnz(), 0x200 | dyn_csc_dtype(m)),
        _ => (0, 0),
    };
    (x.0.as_ptr() as usize, adata.n_obs(), adata.n_vars(), nnz, variant)
}
fn dyn_csr_dtype(m: &DynCsrMatrix) -> u32 {
    match m {
        DynCsrMatrix::I8(_) => SRX_I8 as u32, DynCsrMatrix::I16(_) => SRX_I16 as u32, DynCsrMatrix::I32(_) => SRX_I32 as u32,
        DynCsrMatrix::U8(_) => SRX_U8 as u32, DynCsrMatrix::U16(_) => SRX_U16 as u32, DynCsrMatrix::U32(_) => SRX_U32 as u32,
        DynCsrMatrix::F32(_) => SRX_F32 as u32, DynCsrMatrix::F64(_) => SRX_F64 as u32, _ => 0xff,
    }
}
fn dyn_csc_dtype(m: &DynCscMatrix) -> u32 {
    match m {
        DynCscMatrix::I8(_) => SRX_I8 as u32, DynCscMatrix::I16(_) => SRX_I16 as u32, DynCscMatrix::I32(_) => SRX_I32 as u32,
        DynCscMatrix::U8(_) => SRX_U8 as u32, DynCscMatrix::U16(_) => SRX_U16 as u32, DynCscMatrix::U32(_) => SRX_U32 as u32,
        DynCscMatrix::F32(_) => SRX_F32 as u32, DynCscMatrix::F64(_) => SRX_F64 as u32, _ => 0xff,
    }
}

/// Runs `f` on the resident handle of `adata`, uploading X first when the cache holds another matrix (or nothing).
/// `f` must not call back into the shim's free functions: the cache is mutably borrowed while it runs.
fn with_resident<R>(adata: &IMAnnData, f: impl FnOnce(&mut DeviceX<'static>) -> Result<R>) -> Result<R> {
    with_ctx(|c| {
        let key = x_key(adata);
        TLS.with(|t| {
            let mut slot = t.resident.borrow_mut();
            if slot.as_ref().map_or(true, |s| s.key != key) {
                // the handle about to be dropped may hold the only current values of ANOTHER matrix (lazy mode): they cannot
                // be written back from here (that IMAnnData is not in reach), and dropping them silently would leave its host
                // copy pre-transform for good
                if slot.as_ref().map_or(false, |s| s.host_stale) {
                    bail!("a lazy write-back of another X is pending: call flush() on that IMAnnData first (or invalidate() to discard it)");
                }
                let ctx: &'static Ctx = unsafe { &*(c as *const Ctx) };
                *slot = None;                    // the old handle's HBM is free before the new upload asks for its own
                *slot = Some(Resident { key, _x_elem: adata.x(), dev: DeviceX::upload(ctx, adata)?, host_stale: false, keep_f32: false });
            }
            f(&mut slot.as_mut().expect("resident").dev)
        })
    })
}
/// After an in-place operation on the resident handle: copy back now, or remember that the host copy is stale.
fn after_inplace(adata: &mut IMAnnData, keep_f32: bool) -> Result<()> {
    if TLS.with(|t| t.lazy_writeback.get()) {
        // keep_f32 may only go from true to false while a write-back is pending: normalize_total (-> F64, scale/mod.rs:74-83)
        // followed by log1p on an F32 matrix must come back as F64 with f64 values, as in the reference
        TLS.with(|t| if let Some(s) = t.resident.borrow_mut().as_mut() {
            s.keep_f32 = if s.host_stale { s.keep_f32 && keep_f32 } else { keep_f32 };
            s.host_stale = true;
        });
        return Ok(());
    }
    TLS.with(|t| write_back(adata, &t.resident.borrow().as_ref().expect("resident").dev, keep_f32))?;
    rekey(adata);
    Ok(())
}
/// The write-back may have replaced the variant (-> F64): the cached key follows the element it belongs to.
fn rekey(adata: &IMAnnData) {
    TLS.with(|t| if let Some(s) = t.resident.borrow_mut().as_mut() { s.key = x_key(adata); });
}
/// Is a lazy write-back of THIS matrix pending?
fn host_is_stale(adata: &IMAnnData) -> bool {
    TLS.with(|t| t.resident.borrow().as_ref().map_or(false, |s| {
        s.host_stale && s.key.0 == adata.x().0.as_ptr() as usize
    }))
}
/// Brings the IMAnnData up to date with the device (lazy write-back only; a no-op otherwise).
pub fn flush(adata: &mut IMAnnData) -> Result<()> {
    if !host_is_stale(adata) { return Ok(()); }
    TLS.with(|t| {
        let mut slot = t.resident.borrow_mut();
        let s = slot.as_mut().expect("resident");
        write_back(adata, &s.dev, s.keep_f32)?;
        s.host_stale = false;
        s.keep_f32 = false;
        s.key = x_key(adata);                    // (the variant change keeps the element, its nnz and its shape)
        Ok(())
    })
}
/// The device-side result of a filter becomes the resident handle of the IMAnnData that holds the same subset.
fn adopt(adata: &IMAnnData, dev: DeviceX<'static>) {
    TLS.with(|t| *t.resident.borrow_mut() = Some(Resident { key: x_key(adata), _x_elem: adata.x(), dev, host_stale: false, keep_f32: false }));
}

pub mod statistics_free {
    //! src/memory/statistics/mod.rs:10-103, signatures unchanged.
    use super::*;
    use polars::prelude::{NamedFrom, Series};
    pub fn compute_number(adata: &IMAnnData, direction: Direction) -> anyhow::Result<Vec<u32>> {
        with_resident(adata, |x| x.compute_number(direction))
    }
    pub fn compute_sum(adata: &IMAnnData, direction: Direction) -> anyhow::Result<Vec<f64>> {
        with_resident(adata, |x| x.compute_sum(direction))
    }
    pub fn compute_variance(adata: &IMAnnData, direction: Direction) -> anyhow::Result<Vec<f64>> {
        with_resident(adata, |x| x.compute_variance(direction))
    }
    pub fn compute_min_max(adata: &IMAnnData, direction: Direction) -> anyhow::Result<(Vec<f64>, Vec<f64>)> {
        with_resident(adata, |x| x.compute_min_max(direction))
    }
    pub fn compute_std_dev(adata: &IMAnnData, direction: Direction) -> anyhow::Result<Vec<f64>> {
        with_resident(adata, |x| x.compute_std_dev(direction))
    }

    /// src/memory/statistics/mod.rs:48-72: the reference's own container, filled from one row pass and one column pass.
    pub fn compute_qc_variables(adata: &IMAnnData) -> anyhow::Result<crate::memory::statistics::StatisticsContainer> {
        let (num_per_cell, num_per_gene, expr_per_gene, expr_per_cell, variance_per_gene, variance_per_cell, std_dev_per_cell,
             std_dev_per_gene) = with_resident(adata, |x| x.compute_qc_variables())?;
        Ok(crate::memory::statistics::StatisticsContainer {
            num_per_cell, num_per_gene, expr_per_gene, expr_per_cell, variance_per_gene, variance_per_cell, std_dev_per_cell,
            std_dev_per_gene,
        })
    }
    /// src/memory/statistics/mod.rs:74-103, unchanged but for where the eight vectors come from.
    pub fn qc_vars_inplace(adata: &IMAnnData) -> anyhow::Result<()> {
        let data = compute_qc_variables(adata)?;
        let mut obs_df = adata.obs().get_data();
        let mut var_df = adata.var().get_data();
        obs_df.with_column(Series::from_vec("num_genes_per_cell", data.num_per_cell))?;
        obs_df.with_column(Series::from_vec("sum_expr_per_cell", data.expr_per_cell))?;
        obs_df.with_column(Series::from_vec("var_expr_per_cell", data.variance_per_cell))?;
        obs_df.with_column(Series::from_vec("std_dev_per_cell", data.std_dev_per_cell))?;
        var_df.with_column(Series::from_vec("num_cells_per_gene", data.num_per_gene))?;
        var_df.with_column(Series::from_vec("sum_expr_per_gene", data.expr_per_gene))?;
        var_df.with_column(Series::from_vec("var_expr_per_gene", data.variance_per_gene))?;
        var_df.with_column(Series::from_vec("std_dev_per_gene", data.std_dev_per_gene))?;
        adata.obs().set_data(obs_df)?;
        adata.var().set_data(var_df)?;
        Ok(())
    }
}

/// What `scale_row_csr` / `scale_col_csr` / `log1p_data` leave in X (scale/mod.rs:59-89,141-173, transform/mod.rs:8-62):
/// the values come back from the device and, unless the matrix already is F64 (or F32 under log1p), X is REPLACED by the
/// F64 variant built on the unchanged sparsity pattern — `*csr_matrix = DynCsrMatrix::F64(float_matrix)` (scale/mod.rs:82).
fn write_back(adata: &mut IMAnnData, x: &DeviceX, keep_f32: bool) -> Result<()> {
    let xe = adata.x();
    let mut guard = xe.0.write_inner();
    match guard.deref_mut() {
        AD::CsrMatrix(csr) => {
            let nnz = match csr { DynCsrMatrix::F64(m) => m.nnz(), DynCsrMatrix::F32(m) => m.nnz(), other => other.nnz() };
            match csr {
                DynCsrMatrix::F64(m) => {                                               // in place (:66-73)
                    x.ctx.check(unsafe { srx_matrix_download_values(x.mat, m.values_mut().as_mut_ptr() as *mut c_void, SRX_F64) })
                }
                DynCsrMatrix::F32(m) if keep_f32 => {                                    // f32::ln_1p in place (transform/mod.rs:43-47)
                    x.ctx.check(unsafe { srx_matrix_download_values(x.mat, m.values_mut().as_mut_ptr() as *mut c_void, SRX_F32) })
                }
                other => {                                                              // clone -> f64 -> replace (:74-83)
                    let values = x.download_values_f64(nnz)?;
                    let float_matrix: CsrMatrix<f64> = other.clone().try_into()?;       // the pattern, as the reference obtains it
                    let (offsets, indices, _) = float_matrix.disassemble();
                    *other = DynCsrMatrix::F64(CsrMatrix::try_from_csr_data(x.n_obs, x.n_vars, offsets, indices, values)
                        .map_err(|e| anyhow!("{e}"))?);
                    Ok(())
                }
            }
        }
        AD::CscMatrix(csc) => {                                                          // scale_row_csc / scale_col_csc (:25-57,104-139)
            let nnz = csc.nnz();
            match csc {
                DynCscMatrix::F64(m) => x.ctx.check(unsafe { srx_matrix_download_values(x.mat, m.values_mut().as_mut_ptr() as *mut c_void, SRX_F64) }),
                DynCscMatrix::F32(m) if keep_f32 => x.ctx.check(unsafe { srx_matrix_download_values(x.mat, m.values_mut().as_mut_ptr() as *mut c_void, SRX_F32) }),
                other => {
                    let values = x.download_values_f64(nnz)?;
                    let float_matrix: CscMatrix<f64> = other.clone().try_into()?;
                    let (offsets, indices, _) = float_matrix.disassemble();
                    *other = DynCscMatrix::F64(CscMatrix::try_from_csc_data(x.n_obs, x.n_vars, offsets, indices, values)
                        .map_err(|e| anyhow!("{e}"))?);
                    Ok(())
                }
            }
        }
        _ => bail!("X is neither a CSC nor a CSR matrix"),                               // transform/mod.rs:58
    }
}

pub mod processing_free {
    //! src/memory/processing/mod.rs:303-332, signatures unchanged.
    use super::*;
    pub fn normalize_total_inplace(adata: &mut IMAnnData, target_sum: f64, direction: Direction) -> anyhow::Result<()> {
        with_resident(adata, |x| x.normalize_total_inplace(target_sum, direction))?;
        after_inplace(adata, false)                         // X becomes DynCsrMatrix::F64 whatever it was
    }
    pub fn normalize_total(adata: &IMAnnData, target_sum: f64, direction: Direction) -> anyhow::Result<IMAnnData> {
        // `deep_clone` copies the HOST X: with a lazy write-back pending that is the pre-transform matrix (and a `&IMAnnData`
        // cannot be flushed from here) — the same refusal as the copying filters below
        if host_is_stale(adata) {
            bail!("normalize_total: a lazy write-back of X is pending — call flush(adata) first (or use normalize_total_inplace)");
        }
        let mut new_data = adata.deep_clone();              // :319, as in the reference
        normalize_total_inplace(&mut new_data, target_sum, direction)?;
        flush(&mut new_data)?;                              // a returned copy is always current
        // (the resident handle now belongs to `new_data` and holds its Arc: if the caller drops the result, the next
        //  deep_clone cannot reuse the address, and a later call on `adata` uploads `adata` again)
        Ok(new_data)
    }
    pub fn log1p_transform_inplace(adata: &mut IMAnnData) -> anyhow::Result<()> {
        with_resident(adata, |x| x.log1p_transform_inplace())?;
        after_inplace(adata, true)                          // F32 stays F32, every other dtype becomes F64
    }
    pub fn log1p_transform(adata: &IMAnnData) -> anyhow::Result<IMAnnData> {
        if host_is_stale(adata) {
            bail!("log1p_transform: a lazy write-back of X is pending — call flush(adata) first (or use log1p_transform_inplace)");
        }
        let mut new_data = adata.deep_clone();
        log1p_transform_inplace(&mut new_data)?;
        flush(&mut new_data)?;
        Ok(new_data)
    }

    // ---- src/memory/processing/mod.rs:86-146,245-299, signatures unchanged -------------------------------------------
    // The keep-mask (statistics, interpolated quantiles, limits) and the subset of X come from the device; obs / var and
    // the host copy of X are subset by the reference's own `subset[_inplace]`, and the device-side subset becomes the
    // resident handle of the result, so that the calls which follow (normalise, log1p, PCA) do not upload again.
    use anndata::data::SelectInfoElem;
    use ndarray::Array1;
    pub fn filter_cells_inplace(adata: &mut IMAnnData, lower_lim: FlexValue, upper_lim: FlexValue) -> anyhow::Result<()> {
        let (filtered, keep) = with_resident(adata, |x| x.filter_cells(&lower_lim, &upper_lim))?;
        flush(adata)?;                                      // anndata-memory subsets the HOST copy: it must be current
        let mask = Array1::from_vec(keep);
        let selection = crate::shared::processing::get_select_info_obs(Some(mask.view()))?;
        let selection_refs: Vec<&SelectInfoElem> = selection.iter().collect();
        adata.subset_inplace(selection_refs.as_slice())?;
        adopt(adata, filtered);
        Ok(())
    }
    pub fn filter_cells(adata: &IMAnnData, lower_lim: FlexValue, upper_lim: FlexValue) -> anyhow::Result<IMAnnData> {
        // `subset` copies the HOST X: with a lazy write-back pending it would copy pre-transform values that no later flush
        // repairs (the copy gets a current device handle) — and a `&IMAnnData` cannot be flushed from here
        if host_is_stale(adata) {
            bail!("filter_cells: a lazy write-back of X is pending — call flush(adata) first (or use filter_cells_inplace)");
        }
        let (filtered, keep) = with_resident(adata, |x| x.filter_cells(&lower_lim, &upper_lim))?;
        let mask = Array1::from_vec(keep);
        let selection = crate::shared::processing::get_select_info_obs(Some(mask.view()))?;
        let selection_refs: Vec<&SelectInfoElem> = selection.iter().collect();
        let out = adata.subset(selection_refs.as_slice())?;
        adopt(&out, filtered);
        Ok(out)
    }
    pub fn filter_genes_inplace(adata: &mut IMAnnData, lower_lim: FlexValue, upper_lim: FlexValue) -> anyhow::Result<()> {
        let (filtered, keep) = with_resident(adata, |x| x.filter_genes(&lower_lim, &upper_lim))?;
        flush(adata)?;
        let mask = Array1::from_vec(keep);
        let selection = crate::shared::processing::get_select_info_vars(Some(mask.view()))?;
        let selection_refs: Vec<&SelectInfoElem> = selection.iter().collect();
        adata.subset_inplace(selection_refs.as_slice())?;
        adopt(adata, filtered);
        Ok(())
    }
    pub fn filter_genes(adata: &IMAnnData, lower_lim: FlexValue, upper_lim: FlexValue) -> anyhow::Result<IMAnnData> {
        // `subset` copies the HOST X: with a lazy write-back pending it would copy pre-transform values that no later flush
        // repairs (the copy gets a current device handle) — and a `&IMAnnData` cannot be flushed from here
        if host_is_stale(adata) {
            bail!("filter_genes: a lazy write-back of X is pending — call flush(adata) first (or use filter_genes_inplace)");
        }
        let (filtered, keep) = with_resident(adata, |x| x.filter_genes(&lower_lim, &upper_lim))?;
        let mask = Array1::from_vec(keep);
        let selection = crate::shared::processing::get_select_info_vars(Some(mask.view()))?;
        let selection_refs: Vec<&SelectInfoElem> = selection.iter().collect();
        let out = adata.subset(selection_refs.as_slice())?;
        adopt(&out, filtered);
        Ok(out)
    }

    pub mod dim_red {
        //! src/memory/processing/dim_red/mod.rs:24-121.
        use super::super::*;
        /// dim_red/mod.rs:24-94, signature unchanged.  `svd_mode` selects single_algebra's SVD backend in the reference; the
        /// device solver has none to choose: accepted and ignored, like `n_threads`.
        pub fn pca_inplace<S: SVDImplementation>(anndata: &mut IMAnnData, n_components: Option<usize>, center: Option<bool>,
                                                 scale: Option<bool>, n_threads: Option<usize>,
                                                 feature_selection: &FeatureSelection, _svd_mode: S) -> anyhow::Result<()> {
            // HighlyVariableCol / Randomized / VarianceThreshold: the reference's own host code makes the index list
            // (dim_red/mod.rs:125-134,141-153); HighlyVariable(n) and None go to the device
            // (the host-side selection runs BEFORE the resident handle is borrowed: for VarianceThreshold the reference's
            //  select_features calls statistics::compute_variance, whose body is statistics_free::compute_variance here —
            //  it takes the resident handle itself — and the host code must see current values: flush first)
            let host_selection: Option<Vec<u64>> = match feature_selection {
                FeatureSelection::HighlyVariable(_) | FeatureSelection::None => None,
                other => {
                    flush(anndata)?;
                    Some(crate::memory::processing::dim_red::select_features(anndata, other)?
                        .into_iter().map(|i| i as u64).collect())
                }
            };
            let (scores, evr, selected, n_pc) = with_resident(anndata, |x| match host_selection {
                None => x.pca(n_components, center, scale, n_threads, feature_selection),
                Some(sel) => x.pca_with_selection(n_components, center, scale, Some(sel)),
            })?;
            let transformed = Array2::from_shape_vec((anndata.n_obs(), n_pc), scores)?;      // N x n_pc row-major, as pca.transform returns
            attach_pca_results(anndata, transformed, None, Some(evr), selected, n_pc)
        }

        /// `Pca` after `fit` (src/shared/processing/pca/mod.rs:74), held on the device: `transform` (:156-185) projects the
        /// cells of another IMAnnData into the fitted PC space.  The model owns its device copies: the fitted matrix may be
        /// dropped or re-fitted afterwards.
        pub struct PcaModel { h: *mut SrxPcaModel, genes: Option<Vec<String>> }
        impl Drop for PcaModel { fn drop(&mut self) { unsafe { srx_pca_model_free(self.h) } } }
        /// Feature-map entry of a model gene the query does not have.
        pub const ABSENT: u64 = u64::MAX;
        impl PcaModel {
            /// The model the last `pca_inplace` on `adata` left in HBM (the resident handle's result, device to device).
            pub fn from_adata(adata: &IMAnnData) -> anyhow::Result<PcaModel> {
                let names = adata.var_names().into_vec();
                let mut h: *mut SrxPcaModel = null_mut();
                with_resident(adata, |x| x.ctx.check(unsafe { srx_pca_model_from_result(x.mat, &mut h) }))?;
                let mut m = PcaModel { h, genes: None };
                let (k, _) = m.shape()?;
                let mut sel = vec![0u64; k];
                with_ctx(|c| c.check(unsafe { srx_pca_model_info(m.h, null_mut(), null_mut(), sel.as_mut_ptr()) }))?;
                m.genes = Some(sel.iter().map(|&i| names[i as usize].clone()).collect());
                Ok(m)
            }
            /// A model from its parts: components k x n_pc, mean / std k (as `Pca` keeps them), the fitted matrix's selected
            /// feature ids and gene names (`var_names` of the fitted matrix) for the feature map.
            pub fn from_parts(components: &Array2<f64>, mean: &[f64], std: &[f64], selected: &[usize], var_names: &[String],
                              center: bool, scale: bool) -> anyhow::Result<PcaModel> {
                let (k, n_pc) = components.dim();
                if mean.len() != k || std.len() != k || selected.len() != k {
                    bail!("PcaModel::from_parts: mean, std and the selection need k = {k} entries");
                }
                let comps: Vec<f64> = components.iter().copied().collect();            // row-major k x n_pc
                let sel: Vec<u64> = selected.iter().map(|&i| i as u64).collect();
                let mut h: *mut SrxPcaModel = null_mut();
                with_ctx(|c| c.check(unsafe {
                    srx_pca_model_create(c.0, k as u64, n_pc as u64, comps.as_ptr(), mean.as_ptr(), std.as_ptr(), sel.as_ptr(),
                                         center as i32, scale as i32, &mut h)
                }))?;
                let genes = selected.iter().map(|&i| var_names.get(i).cloned().ok_or_else(|| anyhow!("feature {i} out of bounds")))
                    .collect::<anyhow::Result<Vec<String>>>()?;
                Ok(PcaModel { h, genes: Some(genes) })
            }
            fn shape(&self) -> anyhow::Result<(usize, usize)> {
                let (mut k, mut n_pc) = (0u64, 0u64);
                with_ctx(|c| c.check(unsafe { srx_pca_model_info(self.h, &mut k, &mut n_pc, null_mut()) }))?;
                Ok((k as usize, n_pc as usize))
            }
            /// The query column of each model gene, by name (`ABSENT` where the query lacks it).
            pub fn feature_map(&self, query_names: &[String]) -> anyhow::Result<Vec<u64>> {
                let genes = self.genes.as_ref().ok_or_else(|| anyhow!("the model has no gene names"))?;
                let at: std::collections::HashMap<&str, u64> = query_names.iter().enumerate().map(|(j, n)| (n.as_str(), j as u64)).collect();
                Ok(genes.iter().map(|g| at.get(g.as_str()).copied().unwrap_or(ABSENT)).collect())
            }
            /// Pca::transform (pca/mod.rs:156-185) of the cells of `adata`, X as it is: n_obs x n_pc scores.  The gene axes are
            /// matched by name when they differ; a gene of the model the query lacks contributes its centring term only.
            pub fn transform(&self, adata: &IMAnnData) -> anyhow::Result<Array2<f64>> {
                self.transform_with(adata, None, false)
            }
            /// The same with normalize_total(target_sum, Row) and / or ln_1p applied to the raw values on the fly (X is not
            /// modified).
            pub fn transform_with(&self, adata: &IMAnnData, target_sum: Option<f64>, log1p: bool) -> anyhow::Result<Array2<f64>> {
                let (_, n_pc) = self.shape()?;
                let names = adata.var_names().into_vec();
                let feat = self.feature_map(&names)?;
                let bits = if target_sum.is_some() { SRX_BACKED_NORMALIZE } else { 0 } | if log1p { SRX_BACKED_LOG1P } else { 0 };
                let mut scores = vec![0.0f64; adata.n_obs() * n_pc];
                with_resident(adata, |x| x.ctx.check(unsafe {
                    srx_pca_transform(self.h, x.mat, feat.as_ptr(), target_sum.unwrap_or(0.0), bits as i32,
                                      if scores.is_empty() { null_mut() } else { scores.as_mut_ptr() })
                }))?;
                Ok(Array2::from_shape_vec((adata.n_obs(), n_pc), scores)?)
            }
        }

        /// dim_red/mod.rs:96-121, UNCHANGED (copied call for call so that the module is self-contained): obsm["X_pca"] and,
        /// when loadings are given, varm["PCA_loadings"] with row selected[i] <- loadings row i.
        fn attach_pca_results(anndata: &mut IMAnnData, transformed: Array2<f64>, loadings: Option<Array2<f64>>,
                              _explained_variance_ratio: Option<Vec<f64>>, selected_features: Vec<usize>,
                              n_components: usize) -> anyhow::Result<()> {
            let obsm = anndata.obsm();
            obsm.add_array("X_pca".to_string(), IMArrayElement::new(AD::from(transformed)))?;
            if let Some(loadings) = loadings {
                let varm = anndata.varm();
                let mut full_loadings = Array2::zeros((anndata.n_vars(), n_components));
                for (i, &feature_idx) in selected_features.iter().enumerate() {
                    if i < loadings.nrows() {
                        full_loadings.row_mut(feature_idx).assign(&loadings.row(i));
                    }
                }
                varm.add_array("PCA_loadings".to_string(), IMArrayElement::new(AD::from(full_loadings)))?;
            }
            Ok(())
        }

        /// Exact k-nearest-neighbour graph of the cells in the space of the scores the last PCA left on the device
        /// (srx_knn_result; not in the reference — it stands in front of what the commented-out tsne / tsne_inplace,
        /// dim_red/mod.rs:159-227, would build from obsm["X_pca"]).  Returns (indices n_obs x k, Euclidean distances), every
        /// row ascending by (distance, index); `n_pcs` = 0 uses every component.
        pub fn neighbors(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, include_self: bool)
                         -> anyhow::Result<(Array2<u32>, Array2<f64>)> {
            let (n, k) = (adata.n_obs(), n_neighbors);
            let opts = SrxKnnOpts { k: k as i32, n_dims: n_pcs as i32, include_self: include_self as i32, reserved: 0 };
            let mut idx = vec![0u32; n * k];
            let mut dist = vec![0.0f64; n * k];
            let mut info: SrxKnnInfo = unsafe { std::mem::zeroed() };
            with_resident(adata, |x| x.ctx.check(unsafe {
                srx_knn_result(x.mat, &opts, if idx.is_empty() { null_mut() } else { idx.as_mut_ptr() },
                               if dist.is_empty() { null_mut() } else { dist.as_mut_ptr() }, &mut info)
            }))?;
            Ok((Array2::from_shape_vec((n, k), idx)?, Array2::from_shape_vec((n, k), dist)?))
        }
        /// Neighbours of projected cells (PcaModel::transform output) among the fitted cells' scores: srx_knn_points.
        pub fn neighbors_of(reference: &Array2<f64>, query: &Array2<f64>, n_neighbors: usize)
                            -> anyhow::Result<(Array2<u32>, Array2<f64>)> {
            let ((n_ref, d), (n_q, dq)) = (reference.dim(), query.dim());
            if d != dq {
                bail!("neighbors_of: reference has {d} coordinates, query {dq}");
            }
            let r: Vec<f64> = reference.iter().copied().collect();                 // row-major
            let q: Vec<f64> = query.iter().copied().collect();
            let opts = SrxKnnOpts { k: n_neighbors as i32, n_dims: 0, include_self: 0, reserved: 0 };
            let mut idx = vec![0u32; n_q * n_neighbors];
            let mut dist = vec![0.0f64; n_q * n_neighbors];
            if n_q > 0 {
                with_ctx(|c| c.check(unsafe {
                    srx_knn_points(c.0, r.as_ptr(), n_ref as u64, q.as_ptr(), n_q as u64, d as u64, &opts, idx.as_mut_ptr(),
                                   dist.as_mut_ptr(), null_mut())
                }))?;
            }
            Ok((Array2::from_shape_vec((n_q, n_neighbors), idx)?, Array2::from_shape_vec((n_q, n_neighbors), dist)?))
        }

        /// Approximate k-NN of the cells through an inverted-file index over the resident scores (srx_knn_index_result, then
        /// srx_knn_index_search in the self form without self): the k nearest among the members of the `n_probe` nearest
        /// of `n_lists` lists, exact within them.  0 for `n_lists` / `n_probe` takes the defaults (round(4 sqrt(n)), 20);
        /// `n_pcs` = 0 uses every component.  Returns what `neighbors` returns.
        pub fn neighbors_approx(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, n_lists: usize, n_probe: usize)
                                -> anyhow::Result<(Array2<u32>, Array2<f64>)> {
            let (n, k) = (adata.n_obs(), n_neighbors);
            let iopts = SrxIvfOpts { n_lists: n_lists as i32, train_iters: 10, seed: 0, max_train_points: 0 };
            let opts = SrxKnnOpts { k: k as i32, n_dims: 0, include_self: 0, reserved: 0 };
            let mut idx = vec![0u32; n * k];
            let mut dist = vec![0.0f64; n * k];
            with_resident(adata, |x| {
                let mut ix: *mut SrxKnnIndex = null_mut();
                x.ctx.check(unsafe { srx_knn_index_result(x.mat, n_pcs as i32, &iopts, &mut ix) })?;
                let rc = unsafe {
                    srx_knn_index_search(ix, std::ptr::null(), 0, &opts, n_probe as i32,
                                         if idx.is_empty() { null_mut() } else { idx.as_mut_ptr() },
                                         if dist.is_empty() { null_mut() } else { dist.as_mut_ptr() }, null_mut())
                };
                unsafe { srx_knn_index_free(ix) };
                x.ctx.check(rc)
            })?;
            Ok((Array2::from_shape_vec((n, k), idx)?, Array2::from_shape_vec((n, k), dist)?))
        }
        /// The weighted graph of that approximate list (srx_neighbors_index): the list never leaves the device.
        pub fn neighbors_approx_graph(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, n_lists: usize, n_probe: usize)
                                      -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>)> {
            let iopts = SrxIvfOpts { n_lists: n_lists as i32, train_iters: 10, seed: 0, max_train_points: 0 };
            let opts = SrxKnnOpts { k: n_neighbors as i32, n_dims: 0, include_self: 0, reserved: 0 };
            with_resident(adata, |x| {
                let mut ix: *mut SrxKnnIndex = null_mut();
                x.ctx.check(unsafe { srx_knn_index_result(x.mat, n_pcs as i32, &iopts, &mut ix) })?;
                let mut g: *mut SrxGraph = null_mut();
                let rc = unsafe { srx_neighbors_index(ix, &opts, n_probe as i32, null_mut(), &mut g) };
                unsafe { srx_knn_index_free(ix) };
                x.ctx.check(rc)?;
                let out = graph_to_host(x.ctx, g);
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The index over caller-supplied points (srx_knn_index_points; `centroids` None: trained): its centroids, list
        /// offsets and list members (srx_knn_index_fetch) with the counters of srx_knn_index_info_get.
        pub fn knn_index_of(points: &Array2<f64>, centroids: Option<&Array2<f64>>, n_lists: usize)
                            -> anyhow::Result<(Array2<f64>, Vec<u64>, Vec<u32>, SrxIvfInfo)> {
            let (n, d) = points.dim();
            let p: Vec<f64> = points.iter().copied().collect();                    // row-major
            let c: Option<Vec<f64>> = centroids.map(|c| c.iter().copied().collect());
            let n_lists = centroids.map_or(n_lists, |c| c.dim().0);
            let iopts = SrxIvfOpts { n_lists: n_lists as i32, train_iters: 10, seed: 0, max_train_points: 0 };
            with_ctx(|ctx| {
                let mut ix: *mut SrxKnnIndex = null_mut();
                ctx.check(unsafe {
                    srx_knn_index_points(ctx.0, p.as_ptr(), n as u64, d as u64, &iopts,
                                         c.as_ref().map_or(std::ptr::null(), |v| v.as_ptr()), &mut ix)
                })?;
                let mut info: SrxIvfInfo = unsafe { std::mem::zeroed() };
                let mut rc = unsafe { srx_knn_index_info_get(ix, &mut info) };
                let l = info.n_lists as usize;
                let (mut cent, mut off, mut mem) = (vec![0.0f64; l * d], vec![0u64; l + 1], vec![0u32; n]);
                if rc == 0 {
                    rc = unsafe { srx_knn_index_fetch(ix, cent.as_mut_ptr(), off.as_mut_ptr(), mem.as_mut_ptr()) };
                }
                unsafe { srx_knn_index_free(ix) };
                ctx.check(rc)?;
                Ok((Array2::from_shape_vec((l, d), cent)?, off, mem, info))
            })
        }

        /// The weighted neighbour graph of the cells (srx_neighbors_result): exact k-NN over the resident scores, then
        /// scanpy's `pp.neighbors` weights (umap-learn's fuzzy_simplicial_set restated for rows without self; not compared
        /// with either package) — all on the device.  Returns (distances, connectivities), both n_obs x n_obs CSR.
        pub fn neighbors_graph(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize)
                               -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>)> {
            let opts = SrxKnnOpts { k: n_neighbors as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &opts, null_mut(), &mut g) })?;
                let out = graph_to_host(x.ctx, g);
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The same graph from a k-NN list the caller holds (what `neighbors` / `neighbors_of` return): srx_neighbors_from_knn.
        pub fn connectivities_from_knn(indices: &Array2<u32>, distances: &Array2<f64>)
                                       -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>)> {
            let ((n, k), dd) = (indices.dim(), distances.dim());
            if dd != (n, k) {
                bail!("connectivities_from_knn: indices are {n} x {k}, distances {} x {}", dd.0, dd.1);
            }
            let i: Vec<u32> = indices.iter().copied().collect();                   // row-major
            let d: Vec<f64> = distances.iter().copied().collect();
            with_ctx(|c| {
                let mut g: *mut SrxGraph = null_mut();
                c.check(unsafe { srx_neighbors_from_knn(c.0, i.as_ptr(), d.as_ptr(), n as u64, k as u32, &mut g) })?;
                let out = graph_to_host(c, g);
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// BBKNN (srx_bbknn_result): batch-balanced neighbours over the resident scores, their graph, trimmed (`trim` < 0: the
        /// default 10 * neighbors_within_batch * n_batches; 0: none).  `batch`: one label below `n_batches` per cell.  Returns
        /// (distances, connectivities), both n_obs x n_obs CSR, and the call's counters.  Not compared with the bbknn package.
        pub fn bbknn(adata: &IMAnnData, batch: &[u32], n_batches: u32, neighbors_within_batch: usize, n_pcs: usize, trim: i64)
                     -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>, SrxBbknnInfo)> {
            let opts = SrxBbknnOpts { neighbors_within_batch: neighbors_within_batch as i32, n_dims: n_pcs as i32, trim };
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                let mut info: SrxBbknnInfo = unsafe { std::mem::zeroed() };
                x.ctx.check(unsafe { srx_bbknn_result(x.mat, batch.as_ptr(), n_batches, &opts, &mut info, &mut g) })?;
                let out = graph_to_host(x.ctx, g).map(|(d, c)| (d, c, info));
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// BBKNN's trimming (srx_graph_trim) of the graph of a k-NN list the caller holds: (distances, trimmed connectivities).
        pub fn trimmed_connectivities_from_knn(indices: &Array2<u32>, distances: &Array2<f64>, trim: i64)
                                               -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>, SrxTrimInfo)> {
            let ((n, k), dd) = (indices.dim(), distances.dim());
            if dd != (n, k) {
                bail!("trimmed_connectivities_from_knn: indices are {n} x {k}, distances {} x {}", dd.0, dd.1);
            }
            let i: Vec<u32> = indices.iter().copied().collect();                   // row-major
            let d: Vec<f64> = distances.iter().copied().collect();
            with_ctx(|c| {
                let mut src: *mut SrxGraph = null_mut();
                c.check(unsafe { srx_neighbors_from_knn(c.0, i.as_ptr(), d.as_ptr(), n as u64, k as u32, &mut src) })?;
                let mut g: *mut SrxGraph = null_mut();
                let mut info: SrxTrimInfo = unsafe { std::mem::zeroed() };
                let rc = unsafe { srx_graph_trim(src, trim, &mut info, &mut g) };
                unsafe { srx_graph_free(src) };
                c.check(rc)?;
                let out = graph_to_host(c, g).map(|(d, t)| (d, t, info));
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The options of the shared-nearest-neighbour graph as Seurat's FindNeighbors has them: Jaccard weights, every pair
        /// that shares a neighbour, the cell in its own set, pairs below `prune` dropped.
        pub fn snn_opts(prune: f64) -> SrxSnnOpts {
            SrxSnnOpts { weight: SRX_SNN_JACCARD as i32, pairs: SRX_SNN_PAIRS_SHARED as i32, include_self: 1, reserved: 0, prune }
        }
        /// The SNN graph of the cells (srx_neighbors_result, then srx_snn_graph on the list where it lies): `n_neighbors` is
        /// Seurat's k.param, which counts the cell, so the list has n_neighbors - 1 entries.  Returns (the k-NN distances, the
        /// SNN graph), both n_obs x n_obs CSR, and the call's counters.  Not compared with Seurat, PhenoGraph or scran.
        pub fn neighbors_snn(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, opts: &SrxSnnOpts)
                             -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>, SrxSnnInfo)> {
            if n_neighbors < 2 {
                bail!("neighbors_snn: n_neighbors counts the cell itself, so it is at least 2");
            }
            let kopts = SrxKnnOpts { k: (n_neighbors - 1) as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            with_resident(adata, |x| {
                let mut src: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &kopts, null_mut(), &mut src) })?;
                let mut g: *mut SrxGraph = null_mut();
                let mut info: SrxSnnInfo = unsafe { std::mem::zeroed() };
                let rc = unsafe { srx_snn_graph(src, opts, &mut info, &mut g) };
                unsafe { srx_graph_free(src) };
                x.ctx.check(rc)?;
                let out = graph_to_host(x.ctx, g).map(|(d, c)| (d, c, info));
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The SNN graph of a k-NN list the caller holds (srx_snn_from_knn); distances play no part in it.
        pub fn snn_from_knn(indices: &Array2<u32>, opts: &SrxSnnOpts) -> anyhow::Result<(CsrMatrix<f64>, SrxSnnInfo)> {
            let (n, k) = indices.dim();
            let i: Vec<u32> = indices.iter().copied().collect();                   // row-major
            with_ctx(|c| {
                let mut g: *mut SrxGraph = null_mut();
                let mut info: SrxSnnInfo = unsafe { std::mem::zeroed() };
                c.check(unsafe { srx_snn_from_knn(c.0, i.as_ptr(), std::ptr::null(), n as u64, k as u32, opts, &mut info, &mut g) })?;
                let out = graph_to_host(c, g).map(|(_, snn)| (snn, info));
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The smallest shared count whose Jaccard index reaches `prune` (srx_snn_min_shared: host code, no GPU).
        pub fn snn_min_shared(k: usize, include_self: bool, prune: f64) -> anyhow::Result<u32> {
            let mut s = 0u32;
            match unsafe { srx_snn_min_shared(k as u32, include_self as i32, prune, &mut s) } {
                0 => Ok(s),
                rc => Err(anyhow!("srx_snn_min_shared: status {rc}")),
            }
        }
        /// Louvain communities of the cells (srx_neighbors_result, then srx_louvain on the graph where it lies): k-NN with
        /// `n_neighbors` over the first `n_pcs` resident scores (0 = all), the connectivities, parallel Louvain at
        /// `resolution` — all on the device.  Returns one label per cell, communities numbered by descending size, and Q.
        pub fn louvain(adata: &IMAnnData, resolution: f64) -> anyhow::Result<(Vec<u32>, f64)> {
            louvain_with(adata, resolution, 15, 0)
        }
        pub fn louvain_with(adata: &IMAnnData, resolution: f64, n_neighbors: usize, n_pcs: usize)
                            -> anyhow::Result<(Vec<u32>, f64)> {
            let kopts = SrxKnnOpts { k: n_neighbors as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            let lopts = SrxLouvainOpts { resolution, min_gain: 0.0, max_levels: 0, max_sweeps: 0 };
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &kopts, null_mut(), &mut g) })?;
                let mut ginfo: SrxGraphInfo = unsafe { std::mem::zeroed() };
                let mut info: SrxLouvainInfo = unsafe { std::mem::zeroed() };
                let out = x.ctx.check(unsafe { srx_graph_info_get(g, &mut ginfo) }).and_then(|_| {
                    let mut labels = vec![0u32; ginfo.n as usize];
                    x.ctx.check(unsafe { srx_louvain(g, &lopts, labels.as_mut_ptr(), &mut info) })?;
                    Ok((labels, info.modularity))
                });
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// Louvain communities of a symmetric weighted graph the caller holds (srx_louvain_csr validates it on the device).
        pub fn louvain_csr(w: &CsrMatrix<f64>, resolution: f64) -> anyhow::Result<(Vec<u32>, f64)> {
            let n = w.nrows();
            let indptr: Vec<u64> = w.row_offsets().iter().map(|&v| v as u64).collect();
            let indices: Vec<u32> = w.col_indices().iter().map(|&v| v as u32).collect();
            let lopts = SrxLouvainOpts { resolution, min_gain: 0.0, max_levels: 0, max_sweeps: 0 };
            with_ctx(|c| {
                let mut labels = vec![0u32; n];
                let mut info: SrxLouvainInfo = unsafe { std::mem::zeroed() };
                c.check(unsafe {
                    srx_louvain_csr(c.0, indptr.as_ptr(), indices.as_ptr(), w.values().as_ptr(), n as u64, &lopts,
                                    labels.as_mut_ptr(), &mut info)
                })?;
                Ok((labels, info.modularity))
            })
        }
        /// Labels for new cells from a fitted data set (srx_knn_vote): `indices` is the new cells' k-NN list among the
        /// reference cells (what `neighbors_of` returns), `ref_labels` one label below `n_groups` per reference cell.  Returns
        /// per new cell the most frequent label among its neighbours (ties to the lowest label) and its share of the k.
        pub fn knn_vote(indices: &Array2<u32>, ref_labels: &[u32], n_groups: u32) -> anyhow::Result<(Vec<u32>, Vec<f64>)> {
            let (n, k) = indices.dim();
            let i: Vec<u32> = indices.iter().copied().collect();                   // row-major
            with_ctx(|c| {
                let (mut labels, mut counts) = (vec![0u32; n], vec![0u32; n]);
                c.check(unsafe {
                    srx_knn_vote(c.0, i.as_ptr(), n as u64, k as u32, ref_labels.as_ptr(), ref_labels.len() as u64, n_groups,
                                 labels.as_mut_ptr(), counts.as_mut_ptr())
                })?;
                Ok((labels, counts.iter().map(|&v| v as f64 / k.max(1) as f64).collect()))
            })
        }
        /// New cells placed in a fitted UMAP without refitting it (srx_umap_transform_knn, every default of include/srx.h):
        /// `indices` / `distances` are the new cells' k-NN list among the reference cells (3 <= k <= 64), `ref_embedding` the
        /// reference's `n_ref x dim` layout (dim 2 or 3).  Returns `n_query x dim` and the call's info.
        pub fn umap_transform(indices: &Array2<u32>, distances: &Array2<f64>, ref_embedding: &Array2<f64>)
                              -> anyhow::Result<(Array2<f64>, SrxUmapTransformInfo)> {
            let ((n, k), dd, (n_ref, dim)) = (indices.dim(), distances.dim(), ref_embedding.dim());
            if dd != (n, k) {
                bail!("umap_transform: indices are {n} x {k}, distances {} x {}", dd.0, dd.1);
            }
            let i: Vec<u32> = indices.iter().copied().collect();                   // row-major
            let d: Vec<f64> = distances.iter().copied().collect();
            let y: Vec<f64> = ref_embedding.iter().copied().collect();
            with_ctx(|c| {
                let mut emb = vec![0.0f64; n * dim];
                let mut tout: SrxUmapTransformOut = unsafe { std::mem::zeroed() };
                tout.embedding = emb.as_mut_ptr();
                let mut tinfo: SrxUmapTransformInfo = unsafe { std::mem::zeroed() };
                c.check(unsafe {
                    srx_umap_transform_knn(c.0, i.as_ptr(), d.as_ptr(), n as u64, k as u32, y.as_ptr(), n_ref as u64, dim as u32,
                                           std::ptr::null(), &mut tout, &mut tinfo)
                })?;
                Ok((Array2::from_shape_vec((n, dim), emb).map_err(|e| anyhow!("umap_transform: {e}"))?, tinfo))
            })
        }
        /// The two calls against what lies on the device with a graph handle: the labels of its last srx_louvain
        /// (srx_knn_vote_graph) and the embedding of its last srx_umap (srx_umap_transform_graph, `dim` = that embedding's).
        #[allow(dead_code)]
        fn ingest_on_graph(c: &Ctx, g: *mut SrxGraph, indices: &[u32], distances: &[f64], n: usize, k: usize, dim: usize)
                           -> anyhow::Result<(Vec<u32>, Vec<u32>, Vec<f64>)> {
            let (mut labels, mut counts, mut emb) = (vec![0u32; n], vec![0u32; n], vec![0.0f64; n * dim]);
            c.check(unsafe { srx_knn_vote_graph(g, indices.as_ptr(), n as u64, k as u32, labels.as_mut_ptr(), counts.as_mut_ptr()) })?;
            let mut tout: SrxUmapTransformOut = unsafe { std::mem::zeroed() };
            tout.embedding = emb.as_mut_ptr();
            c.check(unsafe {
                srx_umap_transform_graph(g, indices.as_ptr(), distances.as_ptr(), n as u64, k as u32, dim as u32, std::ptr::null(), &mut tout,
                                         null_mut())
            })?;
            Ok((labels, counts, emb))
        }
        /// The labels the last srx_louvain left with a graph handle (srx_graph_labels_fetch).
        #[allow(dead_code)]
        fn graph_labels(c: &Ctx, g: *mut SrxGraph, n: usize) -> anyhow::Result<Vec<u32>> {
            let mut labels = vec![0u32; n];
            c.check(unsafe { srx_graph_labels_fetch(g, labels.as_mut_ptr()) })?;
            Ok(labels)
        }
        /// What PAGA gives `uns["paga"]`: the tables are `n_groups x n_groups`, row-major; `tree` holds its edges at g < h.
        pub struct Paga {
            pub n_groups: usize,
            pub sizes: Vec<u64>,
            pub out_edges: Vec<u64>,
            pub counts: Vec<u64>,
            pub connectivities: Vec<f64>,
            pub expected: Vec<f64>,
            pub tree: Vec<f64>,
            pub info: SrxPagaInfo,
        }
        /// The buffers of one call: `run` receives the `SrxPagaTables` that points at them and the info to fill.
        fn paga_call(n_groups: usize, run: impl FnOnce(*mut SrxPagaTables, *mut SrxPagaInfo) -> anyhow::Result<()>)
                     -> anyhow::Result<Paga> {
            let gg = n_groups * n_groups;
            let mut p = Paga { n_groups, sizes: vec![0; n_groups], out_edges: vec![0; n_groups], counts: vec![0; gg],
                               connectivities: vec![0.0; gg], expected: vec![0.0; gg], tree: vec![0.0; gg],
                               info: unsafe { std::mem::zeroed() } };
            let mut t = SrxPagaTables { sizes: p.sizes.as_mut_ptr(), out_edges: p.out_edges.as_mut_ptr(), counts: p.counts.as_mut_ptr(),
                                        connectivities: p.connectivities.as_mut_ptr(), expected: p.expected.as_mut_ptr(),
                                        tree: p.tree.as_mut_ptr() };
            run(&mut t, &mut p.info)?;
            Ok(p)
        }
        /// PAGA of the cells' k-NN graph over the communities Louvain finds on it (srx_neighbors_result, srx_louvain, then
        /// srx_paga with the labels where they lie): nothing but the `n_groups x n_groups` tables and the labels comes back.
        pub fn paga(adata: &IMAnnData, resolution: f64, n_neighbors: usize, n_pcs: usize) -> anyhow::Result<(Vec<u32>, Paga)> {
            let kopts = SrxKnnOpts { k: n_neighbors as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            let lopts = SrxLouvainOpts { resolution, min_gain: 0.0, max_levels: 0, max_sweeps: 0 };
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &kopts, null_mut(), &mut g) })?;
                let mut ginfo: SrxGraphInfo = unsafe { std::mem::zeroed() };
                let mut linfo: SrxLouvainInfo = unsafe { std::mem::zeroed() };
                let out = x.ctx.check(unsafe { srx_graph_info_get(g, &mut ginfo) }).and_then(|_| {
                    let mut labels = vec![0u32; ginfo.n as usize];
                    x.ctx.check(unsafe { srx_louvain(g, &lopts, labels.as_mut_ptr(), &mut linfo) })?;
                    let n_groups = (linfo.n_communities as usize).max(1);
                    let p = paga_call(n_groups, |t, info| x.ctx.check(unsafe { srx_paga(g, std::ptr::null(), n_groups as u32, t, info) }))?;
                    Ok((labels, p))
                });
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// PAGA of any directed pattern the caller holds, one label below `n_groups` per row (srx_paga_csr).
        pub fn paga_csr(pattern: &CsrMatrix<f64>, labels: &[u32], n_groups: usize) -> anyhow::Result<Paga> {
            let n = pattern.nrows();
            if labels.len() != n {
                bail!("paga_csr: {} labels for {n} rows", labels.len());
            }
            let indptr: Vec<u64> = pattern.row_offsets().iter().map(|&v| v as u64).collect();
            let indices: Vec<u32> = pattern.col_indices().iter().map(|&v| v as u32).collect();
            with_ctx(|c| paga_call(n_groups, |t, info| {
                c.check(unsafe { srx_paga_csr(c.0, indptr.as_ptr(), indices.as_ptr(), n as u64, labels.as_ptr(), n_groups as u32, t, info) })
            }))
        }
        /// Everything after the counts (host code in the library: no device): `counts` is `n_groups x n_groups`, row-major.
        pub fn paga_from_counts(counts: &[u64], sizes: &[u64]) -> anyhow::Result<Paga> {
            let n_groups = sizes.len();
            if counts.len() != n_groups * n_groups {
                bail!("paga_from_counts: {} counts for {n_groups} groups", counts.len());
            }
            paga_call(n_groups, |t, info| {
                match unsafe { srx_paga_from_counts(counts.as_ptr(), sizes.as_ptr(), n_groups as u32, t, info) } {
                    SRX_OK => Ok(()),
                    rc => Err(anyhow!("srx_paga_from_counts: status {rc}")),
                }
            })
        }
        /// Start positions for a layout from PAGA (srx_paga_init_positions): `pos` is the coarse layout, `n_groups x dim`;
        /// returns `n x dim`, what `umap` takes as a given start.
        pub fn paga_init_positions(labels: &[u32], p: &Paga, pos: &Array2<f64>, seed: u64) -> anyhow::Result<Array2<f64>> {
            let (rows, dim) = pos.dim();
            if rows != p.n_groups {
                bail!("paga_init_positions: pos has {rows} rows for {} groups", p.n_groups);
            }
            let flat: Vec<f64> = pos.iter().copied().collect();                    // row-major
            let mut out = vec![0.0f64; labels.len() * dim];
            with_ctx(|c| c.check(unsafe {
                srx_paga_init_positions(null_mut(), c.0, labels.as_ptr(), labels.len() as u64, p.n_groups as u32,
                                        p.connectivities.as_ptr(), flat.as_ptr(), dim as u32, seed, out.as_mut_ptr())
            }))?;
            Array2::from_shape_vec((labels.len(), dim), out).map_err(|e| anyhow!("paga_init_positions: {e}"))
        }
        /// ForceAtlas2 layout of the cells' k-NN connectivities, what `sc.tl.draw_graph(layout="fa")` gives (srx_neighbors_result,
        /// then srx_draw_graph on the graph where it lies, every default of include/srx.h: 500 iterations, theta 1.2).  `init`:
        /// `n x 2` start positions (what `paga_init_positions` returns), or None for the hashed start of `seed`.
        pub fn draw_graph(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, init: Option<&Array2<f64>>, seed: u64)
                          -> anyhow::Result<(Array2<f64>, SrxFa2Info)> {
            let kopts = SrxKnnOpts { k: n_neighbors as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            let start: Option<Vec<f64>> = init.map(|y| y.iter().copied().collect());    // row-major
            let fopts = SrxFa2Opts { theta: 1.2, scaling_ratio: 2.0, gravity: 1.0, jitter_tolerance: 1.0, seed, n_iter: 500,
                                     stop_after: 0, levels: 0, init: if start.is_some() { 0 } else { 1 }, strong_gravity: 0, linlog: 0 };
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &kopts, null_mut(), &mut g) })?;
                let mut ginfo: SrxGraphInfo = unsafe { std::mem::zeroed() };
                let mut info: SrxFa2Info = unsafe { std::mem::zeroed() };
                let out = x.ctx.check(unsafe { srx_graph_info_get(g, &mut ginfo) }).and_then(|_| {
                    let n = ginfo.n as usize;
                    if let Some(s) = &start {
                        if s.len() != n * 2 {
                            bail!("draw_graph: the start has {} values for {n} x 2", s.len());
                        }
                    }
                    let mut y = vec![0.0f64; n * 2];
                    x.ctx.check(unsafe {
                        srx_draw_graph(g, &fopts, start.as_ref().map_or(std::ptr::null(), |s| s.as_ptr()), y.as_mut_ptr(), &mut info)
                    })?;
                    Ok((Array2::from_shape_vec((n, 2), y).map_err(|e| anyhow!("draw_graph: {e}"))?, info))
                });
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The same for a symmetric weighted graph the caller holds (srx_draw_graph_csr validates it on the device), from the
        /// hashed start of `seed`.
        pub fn draw_graph_csr(w: &CsrMatrix<f64>, seed: u64) -> anyhow::Result<(Array2<f64>, SrxFa2Info)> {
            let n = w.nrows();
            let indptr: Vec<u64> = w.row_offsets().iter().map(|&v| v as u64).collect();
            let indices: Vec<u32> = w.col_indices().iter().map(|&v| v as u32).collect();
            let fopts = SrxFa2Opts { theta: 1.2, scaling_ratio: 2.0, gravity: 1.0, jitter_tolerance: 1.0, seed, n_iter: 500,
                                     stop_after: 0, levels: 0, init: 1, strong_gravity: 0, linlog: 0 };
            with_ctx(|c| {
                let mut y = vec![0.0f64; n * 2];
                let mut info: SrxFa2Info = unsafe { std::mem::zeroed() };
                c.check(unsafe {
                    srx_draw_graph_csr(c.0, indptr.as_ptr(), indices.as_ptr(), w.values().as_ptr(), n as u64, &fopts, std::ptr::null(),
                                       y.as_mut_ptr(), &mut info)
                })?;
                Ok((Array2::from_shape_vec((n, 2), y).map_err(|e| anyhow!("draw_graph_csr: {e}"))?, info))
            })
        }
        /// The speed rule of a ForceAtlas2 iteration on the host (srx_fa2_speed; no GPU): the new (speed, efficiency).
        pub fn fa2_speed(n: u64, swing: f64, traction: f64, jitter_tolerance: f64, speed: f64, efficiency: f64)
                         -> anyhow::Result<(f64, f64)> {
            let (mut s, mut e) = (speed, efficiency);
            if unsafe { srx_fa2_speed(n, swing, traction, jitter_tolerance, &mut s, &mut e) } != 0 {
                bail!("fa2_speed: refused (n = {n}, swing = {swing}, traction = {traction})");
            }
            Ok((s, e))
        }
        /// Moran's I and Geary's C per gene with their z-scores under normality; a constant gene has NaN statistics.
        pub struct Autocorr {
            pub morans_i: Vec<f64>,
            pub gearys_c: Vec<f64>,
            pub z_i: Vec<f64>,
            pub z_c: Vec<f64>,
            pub info: SrxAutocorrInfo,
        }
        /// The buffers of one call: `run` receives the `SrxAutocorrOut` that points at them (the tables are not asked for).
        fn autocorr_call(n_genes: usize, run: impl FnOnce(*mut SrxAutocorrOut, *mut SrxAutocorrInfo) -> anyhow::Result<()>)
                         -> anyhow::Result<Autocorr> {
            let mut r = Autocorr { morans_i: vec![0.0; n_genes], gearys_c: vec![0.0; n_genes], z_i: vec![0.0; n_genes],
                                   z_c: vec![0.0; n_genes], info: unsafe { std::mem::zeroed() } };
            let mut o: SrxAutocorrOut = unsafe { std::mem::zeroed() };
            o.morans_i = r.morans_i.as_mut_ptr();
            o.gearys_c = r.gearys_c.as_mut_ptr();
            o.z_i = r.z_i.as_mut_ptr();
            o.z_c = r.z_c.as_mut_ptr();
            run(&mut o, &mut r.info)?;
            Ok(r)
        }
        /// Which genes vary smoothly along the cells' k-NN graph (srx_neighbors_result, then srx_autocorr with the
        /// connectivities where they lie): four numbers per gene come back, nothing per cell.
        pub fn gene_autocorr(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize) -> anyhow::Result<Autocorr> {
            let kopts = SrxKnnOpts { k: n_neighbors as i32, n_dims: n_pcs as i32, include_self: 0, reserved: 0 };
            let n_genes = adata.n_vars();
            with_resident(adata, |x| {
                let mut g: *mut SrxGraph = null_mut();
                x.ctx.check(unsafe { srx_neighbors_result(x.mat, &kopts, null_mut(), &mut g) })?;
                let out = autocorr_call(n_genes, |o, info| x.ctx.check(unsafe { srx_autocorr(x.mat, g, std::ptr::null(), o, info) }));
                unsafe { srx_graph_free(g) };
                out
            })
        }
        /// The same on any symmetric weighted graph over the cells the caller holds (srx_autocorr_csr).
        pub fn autocorr_csr(adata: &IMAnnData, graph: &CsrMatrix<f64>) -> anyhow::Result<Autocorr> {
            let n = graph.nrows();
            let n_genes = adata.n_vars();
            let indptr: Vec<u64> = graph.row_offsets().iter().map(|&v| v as u64).collect();
            let indices: Vec<u32> = graph.col_indices().iter().map(|&v| v as u32).collect();
            with_resident(adata, |x| autocorr_call(n_genes, |o, info| {
                x.ctx.check(unsafe { srx_autocorr_csr(x.mat, indptr.as_ptr(), indices.as_ptr(), graph.values().as_ptr(), n as u64,
                                                      std::ptr::null(), o, info) })
            }))
        }
        /// The eight fixed-point scales from `info`'s n, nnz, max_abs, max_weight and max_degree (srx_autocorr_scales: host code).
        pub fn autocorr_scales(mut info: SrxAutocorrInfo) -> anyhow::Result<SrxAutocorrInfo> {
            match unsafe { srx_autocorr_scales(&mut info) } {
                SRX_OK => Ok(info),
                rc => Err(anyhow!("srx_autocorr_scales: status {rc}")),
            }
        }
        /// The statistics from the five integer tables (host code in the library: no device); `info` carries n, the scales and
        /// the graph's integer sums.
        pub fn autocorr_from_tables(tables: [&[i64]; 5], info: SrxAutocorrInfo) -> anyhow::Result<Autocorr> {
            let n_genes = tables[0].len();
            if tables.iter().any(|t| t.len() != n_genes) {
                bail!("autocorr_from_tables: five tables of one length expected");
            }
            let mut filled = info;
            let mut r = autocorr_call(n_genes, |o, _| {
                match unsafe { srx_autocorr_from_tables(tables[0].as_ptr(), tables[1].as_ptr(), tables[2].as_ptr(), tables[3].as_ptr(),
                                                        tables[4].as_ptr(), n_genes as u64, &mut filled, o) } {
                    SRX_OK => Ok(()),
                    rc => Err(anyhow!("srx_autocorr_from_tables: status {rc}")),
                }
            })?;
            r.info = filled;                                              // w, s1, s2, E, Var, genes_constant as the library filled them
            Ok(r)
        }
        fn graph_to_host(c: &Ctx, g: *mut SrxGraph) -> anyhow::Result<(CsrMatrix<f64>, CsrMatrix<f64>)> {
            let mut info: SrxGraphInfo = unsafe { std::mem::zeroed() };
            c.check(unsafe { srx_graph_info_get(g, &mut info) })?;
            let n = info.n as usize;
            let mut fetch = |which: i32, nnz: usize| -> anyhow::Result<CsrMatrix<f64>> {
                let mut indptr = vec![0u64; n + 1];
                let mut indices = vec![0u32; nnz];
                let mut data = vec![0.0f64; nnz];
                c.check(unsafe { srx_graph_fetch(g, which, indptr.as_mut_ptr(), indices.as_mut_ptr(), data.as_mut_ptr()) })?;
                CsrMatrix::try_from_csr_data(n, n, indptr.into_iter().map(|v| v as usize).collect(),
                                             indices.into_iter().map(|v| v as usize).collect(), data)
                    .map_err(|e| anyhow!("graph: {e}"))
            };
            Ok((fetch(SRX_GRAPH_DISTANCES, info.nnz_distances as usize)?,
                fetch(SRX_GRAPH_CONNECTIVITIES, info.nnz_connectivities as usize)?))
        }
    }
}

pub mod backed_statistics_free {
    //! src/backed/statistics/mod.rs:5-45, signatures unchanged.  `ComputationMode::Chunked(size)` walks anndata's row-chunk
    //! iterator and hands every chunk to the session as a row tile (the device keeps the per-gene accumulators and writes
    //! the per-cell results at the tile's GLOBAL row offset — the reference's chunk loop indexes them by the chunk-local
    //! row, csr.rs:57-62,126-131); `Whole` reads X once, as the reference does.
    use super::*;
    use anndata::{AnnData, AnnDataOp, ArrayElemOp, Backend};
    use crate::shared::ComputationMode;

    struct Session<'c> { ctx: &'c Ctx, h: *mut SrxBacked }
    impl Drop for Session<'_> { fn drop(&mut self) { unsafe { srx_backed_destroy(self.h) } } }

    /// One sweep over the chunks: per-cell counts / sums land in `row_num` / `row_sum`, the per-gene ones stay in the session.
    fn sweep<B: Backend>(c: &Ctx, adata: &AnnData<B>, size: usize, row_num: Option<&mut [u32]>, row_sum: Option<&mut [f64]>)
                         -> Result<(Vec<u64>, Vec<f64>)> {
        let n_vars = adata.n_vars();
        let mut h = null_mut();
        c.check(unsafe { srx_backed_create(c.0, n_vars as u64, SRX_STORE_AUTO, &mut h) })?;
        let s = Session { ctx: c, h };
        let (mut num_p, mut sum_p) = (row_num.map_or(null_mut(), |v| v.as_mut_ptr()), row_sum.map_or(null_mut(), |v| v.as_mut_ptr()));
        for (chunk, start, end) in adata.x().iter::<ArrayData>(size) {
            let d = match &chunk {
                ArrayData::CsrMatrix(DynCsrMatrix::F64(m)) => csr_descriptor!(m, SRX_F64),
                ArrayData::CsrMatrix(DynCsrMatrix::F32(m)) => csr_descriptor!(m, SRX_F32),
                ArrayData::CsrMatrix(DynCsrMatrix::U32(m)) => csr_descriptor!(m, SRX_U32),
                ArrayData::CsrMatrix(DynCsrMatrix::I32(m)) => csr_descriptor!(m, SRX_I32),
                ArrayData::CsrMatrix(DynCsrMatrix::U16(m)) => csr_descriptor!(m, SRX_U16),
                ArrayData::CsrMatrix(DynCsrMatrix::I16(m)) => csr_descriptor!(m, SRX_I16),
                ArrayData::CsrMatrix(DynCsrMatrix::U8(m)) => csr_descriptor!(m, SRX_U8),
                ArrayData::CsrMatrix(DynCsrMatrix::I8(m)) => csr_descriptor!(m, SRX_I8),
                _ => bail!("X is not a CSR matrix"),
            };
            s.ctx.check(unsafe { srx_backed_stats_tile(s.h, &d, 0.0, 0, num_p, sum_p) })?;      // transform 0: the raw values
            let rows = end - start;
            if !num_p.is_null() { num_p = unsafe { num_p.add(rows) }; }
            if !sum_p.is_null() { sum_p = unsafe { sum_p.add(rows) }; }
        }
        let (mut cnt, mut sum) = (vec![0u64; n_vars], vec![0f64; n_vars]);
        let mut n_rows = 0u64;
        s.ctx.check(unsafe { srx_backed_moments(s.h, cnt.as_mut_ptr(), sum.as_mut_ptr(), null_mut(), &mut n_rows) })?;
        Ok((cnt, sum))
    }

    pub fn compute_number<B: Backend>(adata: AnnData<B>, direction: Direction, mode: ComputationMode) -> anyhow::Result<Vec<u32>> {
        let size = match mode { ComputationMode::Chunked(size) => size, ComputationMode::Whole => adata.n_obs().max(1) };
        with_ctx(|c| match direction {
            Direction::Row => {
                let mut v = vec![0u32; adata.n_obs()];
                sweep(c, &adata, size, Some(&mut v), None)?;
                Ok(v)
            }
            Direction::Column => Ok(sweep(c, &adata, size, None, None)?.0.into_iter().map(|n| n as u32).collect()),
        })
    }
    pub fn compute_sum<B: Backend>(adata: AnnData<B>, direction: Direction, mode: ComputationMode) -> anyhow::Result<Vec<f64>> {
        let size = match mode { ComputationMode::Chunked(size) => size, ComputationMode::Whole => adata.n_obs().max(1) };
        with_ctx(|c| match direction {
            Direction::Row => {
                let mut v = vec![0f64; adata.n_obs()];
                sweep(c, &adata, size, None, Some(&mut v))?;
                Ok(v)
            }
            Direction::Column => Ok(sweep(c, &adata, size, None, None)?.1),
        })
    }
}
