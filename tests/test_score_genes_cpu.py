"""Gene-set scores without a GPU: srx_score_genes_controls (pure host code) against pandas' rank, against the Python restatement
(score_genes_ref.py) and against the `fractions` known answer (golden/kat_score_genes.json); every refusal of that call with its
message; the hash of hash.hpp against Python ints; the host logic of the Python helpers (phase rule, name resolution); the new
symbols bound in every layer with the struct layout gcc gives them; the gfx950 listings of the kernels of gene_sets.hip free of
spills, and no floating-point atomic in the file."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import score_genes_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_gene_list_sums", "srx_score_genes_controls", "srx_score_genes")
KAT = json.load(open(os.path.join(S.GOLD, "kat_score_genes.json")))


def F():
    from singlerust_amd import _ffi
    return _ffi


def raw_controls(mean, sets, pool=None, ctrl_size=0, n_bins=0, seed=0, as_ref=-1, capacity=None, opts=True):
    """(rc, message, ctrl lists, cut): the C call with outputs pre-filled with a mark, so that a refusal can be seen to write nothing"""
    f = F()
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    ptr = np.zeros(len(sets) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.uint64) for s in sets] + [np.zeros(1, dtype=np.uint64)]))
    pool_a = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint64)
    cap = 4 * mean.size * max(len(sets), 1) + 8 if capacity is None else capacity
    cptr, cg, cut = np.full(len(sets) + 1, 77, dtype=np.uint64), np.full(max(cap, 1), 77, dtype=np.uint64), np.full(mean.size, 77, dtype=np.uint32)
    o = f.ScoreGenesOpts(ctrl_size, n_bins, seed, as_ref, 0)
    rc = f.lib().srx_score_genes_controls(f.ptr(mean), mean.size, None if pool_a is None else f.ptr(pool_a), 0 if pool_a is None else pool_a.size,
                                          f.ptr(ptr), f.ptr(flat), len(sets), C.byref(o) if opts else None, f.ptr(cptr), f.ptr(cg), cap, f.ptr(cut))
    msg = (f.lib().srx_last_error(None) or b"").decode()
    if rc != 0:
        assert np.all(cptr == 77) and np.all(cg == 77) and np.all(cut == 77), "a refused call wrote to its outputs"
        return rc, msg, None, None
    return rc, msg, [cg[int(cptr[s]):int(cptr[s + 1])].copy() for s in range(len(sets))], cut


def tied_means(P, seed=3):
    """P means with ties, zeros and -0.0: genes 0 and 1 are 0.0 and -0.0 (one rank), the rest hashed onto a few levels"""
    m = np.array([(S.mix64(seed * 7919 + j) % max(P // 3, 2)) * 0.25 for j in range(P)], dtype=np.float64)
    m[:2] = [0.0, -0.0][:P]
    return m


# ---- bins ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [2, 5, 25])
@pytest.mark.parametrize("P", [1, 12, 24, 25, 1000])
def test_cuts_are_pandas_rank_min_over_n_items(P, n_bins):
    import pandas as pd
    mean = tied_means(P)
    n_items = int(np.round(P / (n_bins - 1)))
    rc, msg, ctrl, cut = raw_controls(mean, [[0]], ctrl_size=50, n_bins=n_bins)
    if n_items == 0:
        assert rc == F().E_ARG and "n_items" in msg
        return
    if P == 1:                                                  # the only gene is the set: nothing is left for a control
        assert rc == F().E_ARG and "control list of set 0 is empty" in msg
        return
    assert rc == 0, msg
    want = (pd.Series(mean).rank(method="min").astype(np.int64) // n_items).to_numpy()
    assert np.array_equal(cut.astype(np.int64), want)
    assert cut[0] == cut[1]                                     # -0.0 == 0.0
    assert np.array_equal(cut, S.cuts(mean, None, n_bins)[0])


@pytest.mark.parametrize("case", KAT["n_items_ties"], ids=lambda c: "P%d-bins%d" % (c["P"], c["n_bins"]))
def test_n_items_rounds_ties_to_even(case):
    P, n_bins, n_items = case["P"], case["n_bins"], case["n_items"]
    mean = np.arange(P, dtype=np.float64)
    mean[1] = 0.0                                               # one tie, so that set [0] has a control
    rc, msg, _, cut = raw_controls(mean, [[0]], ctrl_size=50, n_bins=n_bins)
    if n_items == 0:
        assert rc == F().E_ARG and "n_items = rint(%d / %d) = 0" % (P, n_bins - 1) in msg
        return
    assert rc == 0, msg
    ranks = np.array([1, 1] + list(range(3, P + 1)))
    assert np.array_equal(cut, ranks // n_items)


def test_known_answer_bins_and_controls():
    assert KAT["n_items"] == 2 and KAT["ranks"] == [1, 1, 3, 4, 5, 6, 7, 8] and KAT["cuts"] == [0, 0, 1, 2, 2, 3, 3, 4]   # srx.h's example
    sets = [KAT["sets"]["a"], KAT["sets"]["b"]]
    rc, msg, ctrl, cut = raw_controls(KAT["means"], sets, ctrl_size=KAT["ctrl_size"], n_bins=KAT["n_bins"])
    assert rc == 0, msg
    assert cut.tolist() == KAT["cuts"]
    assert [c.tolist() for c in ctrl] == [KAT["controls"]["a"], KAT["controls"]["b"]]
    ref = S.controls(KAT["means"], sets, None, KAT["ctrl_size"], KAT["n_bins"])
    assert [c.tolist() for c in ref] == [KAT["controls"]["a"], KAT["controls"]["b"]]


# ---- the control lists ------------------------------------------------------------------------------------------------------------------
CTRL_SETS = [[0, 5, 17, 30, 31], [2], [100, 101, 102, 150, 199, 3]]


@pytest.mark.parametrize("as_ref", [1, 0])
@pytest.mark.parametrize("ctrl_size", [3, 8, 50])              # bins of 200 / 24 = 8 genes: larger than, equal to, smaller than ctrl_size
@pytest.mark.parametrize("pooled", [False, True])
def test_control_lists_equal_the_reference(pooled, ctrl_size, as_ref):
    G = 200
    mean = np.array([(S.mix64(11 + j) >> 11) / 2.0 ** 53 * 4 for j in range(G)], dtype=np.float64)
    pool = None
    if pooled:                                                  # every gene but a few, in no order; the sets' genes stay in
        keep = sorted(set(range(G)) - {7, 8, 9, 60, 61, 120, 198}, key=lambda j: S.mix64(5 + j))
        pool = np.array(keep, dtype=np.uint64)
    rc, msg, ctrl, cut = raw_controls(mean, CTRL_SETS, pool, ctrl_size, 25, 9, as_ref)
    assert rc == 0, msg
    ref = S.controls(mean, CTRL_SETS, pool, ctrl_size, 25, 9, bool(as_ref))
    n_items = S.n_items_of(G if pool is None else pool.size, 25)
    assert n_items == 8
    for s, (a, b) in enumerate(zip(ctrl, ref)):
        assert np.array_equal(a, b), s
        assert np.all(np.diff(a.astype(np.int64)) > 0) and not set(a.tolist()) & set(CTRL_SETS[s])
        n_cuts = len({int(cut[g]) for g in CTRL_SETS[s]})
        assert len(a) <= ctrl_size * min(len(CTRL_SETS[s]), (G if pool is None else pool.size) // n_items + 1) and n_cuts >= 1
    if pooled:
        assert np.all(cut[[7, 8, 9, 60, 61, 120, 198]] == S.NOT_IN_POOL)
    if ctrl_size == 3 and not as_ref:                           # the hash decided: set 1 has one bin of at least 6 other genes
        assert len(ctrl[1]) == 3


def test_sets_scored_together_equal_sets_scored_alone():
    G = 300
    mean = np.array([(S.mix64(23 + j) % 40) * 0.125 for j in range(G)], dtype=np.float64)
    for as_ref in (1, 0):
        rc, msg, together, _ = raw_controls(mean, CTRL_SETS, None, 4, 25, 5, as_ref)
        assert rc == 0, msg
        for s, genes in enumerate(CTRL_SETS):
            rc, msg, alone, _ = raw_controls(mean, [genes], None, 4, 25, 5, as_ref)
            assert rc == 0 and np.array_equal(alone[0], together[s])
    # and the seed matters
    a = raw_controls(mean, CTRL_SETS, None, 4, 25, 5)[2]
    b = raw_controls(mean, CTRL_SETS, None, 4, 25, 6)[2]
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_defaults_are_50_controls_and_25_bins():
    G = 2400
    mean = np.array([(S.mix64(31 + j) >> 11) / 2.0 ** 53 for j in range(G)], dtype=np.float64)
    sets = [[1, 2, 3]]
    for kw in (dict(opts=False), dict(ctrl_size=0, n_bins=0, seed=0, as_ref=-1)):
        rc, msg, ctrl, _ = raw_controls(mean, sets, **kw)
        assert rc == 0, msg
        assert np.array_equal(ctrl[0], S.controls(mean, sets, None, 50, 25, 0, True)[0])


# ---- the hash -------------------------------------------------------------------------------------------------------------------------------
def test_hash_hpp_key_equals_the_python_hash(tmp_path):
    """hash.hpp compiled as host code: key_j = mix64(seed + kGold64 (j + 1)) for a few (seed, j), the wrap-around included."""
    cases = [(0, 0), (0, 1), (9, 27999), (2 ** 64 - 1, 5), (0x0123456789ABCDEF, 2 ** 40)]
    prog = ('#define __host__\n#define __device__\n#define __forceinline__ inline\n#include <cstdio>\n#include "hash.hpp"\nint main() {\n'
            + "".join('    std::printf("%%llu\\n", (unsigned long long)srx::mix64(%dull + srx::kGold64 * (%dull + 1)));\n' % c for c in cases)
            + "    return 0;\n}\n")
    src, exe = str(tmp_path / "h.cpp"), str(tmp_path / "h")
    open(src, "w").write(prog)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "singlerust_amd", "csrc"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [S.key(seed, j) for seed, j in cases]
    assert S.mix64(0) == 0 and S.mix64(S.GOLD64) == 0xE220A8397B1DCDAF     # splitmix64's first output from state 0


def test_the_kept_controls_are_the_smallest_keys():
    """one bin of 40 genes (n_bins = 2): ctrl_size = k keeps the k smallest (key, gene) of the 38 candidates"""
    G, seed = 40, 12345
    mean = np.arange(G, dtype=np.float64)
    order = sorted(range(1, G - 1), key=lambda j: (S.key(seed, j), j))          # rank 40 // 40 = 1: the last gene has a bin of its own
    for k in (1, 2, 17, 38):
        rc, msg, ctrl, cut = raw_controls(mean, [[0]], None, k, 2, seed, 0)
        assert rc == 0, msg
        assert cut[:-1].max() == 0 and cut[-1] == 1
        assert ctrl[0].tolist() == sorted(order[:k])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_controls_with_its_message():
    f = F()
    G = 48
    mean = np.arange(G, dtype=np.float64)
    mean[1] = 0.0
    ok = dict(ctrl_size=50, n_bins=5)
    assert raw_controls(mean, [[0, 4]], **ok)[0] == 0
    cases = [
        (dict(mean=mean, sets=[[0]], ctrl_size=50, n_bins=1), "n_bins = 1"),
        (dict(mean=mean, sets=[[0]], pool=[0, 1, 2, 48], **ok), "pool gene 48 is not below 48"),
        (dict(mean=mean, sets=[[0]], pool=[0, 1, 2, 1], **ok), "gene 1 is repeated in the pool"),
        (dict(mean=mean, sets=[[0]], pool=[0], **ok), "n_items"),
        (dict(mean=np.where(np.arange(G) == 7, np.nan, mean), sets=[[0]], **ok), "the mean of gene 7 is not finite"),
        (dict(mean=np.where(np.arange(G) == 9, np.inf, mean), sets=[[0]], **ok), "the mean of gene 9 is not finite"),
        (dict(mean=mean, sets=[[0], []], **ok), "set 1 is empty"),
        (dict(mean=mean, sets=[[0, 48]], **ok), "gene index 48 of set 0 is not below 48"),
        (dict(mean=mean, sets=[[0], [3, 5, 3]], **ok), "gene 3 is repeated in set 1"),
        (dict(mean=mean, sets=[[0, 4]], pool=list(range(0, 4)) + list(range(5, 48)), **ok), "gene 4 of a set is not in the pool"),
        (dict(mean=mean, sets=[[0, 1], list(range(48))], **ok), "the control list of set 1 is empty"),
        (dict(mean=mean, sets=[[0, 4]], capacity=3, **ok), "capacity is 3"),
    ]
    for kw, text in cases:
        rc, msg, _, _ = raw_controls(kw.pop("mean"), kw.pop("sets"), **kw)
        assert rc == f.E_ARG and text in msg, (text, rc, msg)
    # a non-finite mean OUTSIDE the pool is not looked at
    assert raw_controls(np.where(np.arange(G) == 40, np.nan, mean), [[0]], pool=list(range(40)), **ok)[0] == 0
    # NULL arrays, no set, a set_ptr that does not start at 0 or that decreases
    lib, one = f.lib(), np.zeros(4, dtype=np.uint64)
    p = f.ptr(one)
    sp, sg = np.array([0, 1], dtype=np.uint64), np.array([0], dtype=np.uint64)
    args = [f.ptr(mean), G, None, 0, f.ptr(sp), f.ptr(sg), 1, None, p, p, 4, None]
    for null_at in (0, 4, 5, 8, 9):
        a = list(args)
        a[null_at] = None
        assert lib.srx_score_genes_controls(*a) == f.E_ARG and b"null array" in lib.srx_last_error(None)
    a = list(args)
    a[3] = 2                                                   # n_pool > 0 without a pool
    assert lib.srx_score_genes_controls(*a) == f.E_ARG and b"null array" in lib.srx_last_error(None)
    a = list(args)
    a[6] = 0
    assert lib.srx_score_genes_controls(*a) == f.E_ARG and b"no set" in lib.srx_last_error(None)
    for bad, text in ((np.array([1, 2], dtype=np.uint64), b"set_ptr[0] = 1"), (np.array([0, 2, 1], dtype=np.uint64), b"set_ptr decreases at set 1")):
        a = list(args)
        a[4], a[5], a[6] = f.ptr(bad), f.ptr(np.array([0, 2, 3], dtype=np.uint64)), bad.size - 1
        assert lib.srx_score_genes_controls(*a) == f.E_ARG and text in lib.srx_last_error(None)
    assert np.all(one == 0)


def test_capacity_bound_of_the_header_is_enough():
    from singlerust_amd.memory.processing import score
    G = 500
    mean = np.array([(S.mix64(3 + j) % 97) * 0.5 for j in range(G)], dtype=np.float64)
    for ctrl_size, n_bins in ((50, 25), (5, 25), (50, 2), (1, 5)):
        cap = score.control_capacity(CTRL_SETS, ctrl_size, n_bins, G)
        rc, msg, ctrl, _ = raw_controls(mean, CTRL_SETS, None, ctrl_size, n_bins, capacity=cap)
        assert rc == 0, msg
        n_items = S.n_items_of(G, n_bins)
        for s, c in zip(CTRL_SETS, ctrl):
            assert len(c) <= ctrl_size * min(len(s), G // n_items + 1)
        lists, _ = score.score_genes_controls(mean, CTRL_SETS, ctrl_size, n_bins)
        assert all(np.array_equal(a, b) for a, b in zip(lists, ctrl))


# ---- the Python helpers' host logic ------------------------------------------------------------------------------------------------------------
def test_phase_rule_is_scanpys():
    from singlerust_amd.memory.processing import cell_cycle_phase
    s = np.array([0.5, 0.1, -0.1, -0.2, 0.3, -0.1, 0.0, -0.3])
    g = np.array([0.1, 0.5, -0.2, -0.1, 0.3, 0.2, 0.0, 0.0])
    want = ["S", "G2M", "G1", "G1", "S", "G2M", "S", "G2M"]
    assert cell_cycle_phase(s, g).tolist() == want == S.phase(s, g).tolist()


def test_names_are_resolved_and_missing_names_dropped():
    from singlerust_amd.memory.processing import score
    names = ["MCM5", "PCNA", "TYMS", "FEN1", "PCNA"]            # a duplicated var name resolves to its first place
    idx, dropped = score.resolve_genes(names, ["PCNA", "nope", "MCM5", "PCNA", "Mlf1ip"], 5)
    assert idx.tolist() == [1, 0] and idx.dtype == np.uint64 and dropped == ["nope", "Mlf1ip"]
    idx, dropped = score.resolve_genes(names, np.array([True, False, False, True, False]), 5)
    assert idx.tolist() == [0, 3] and dropped == []
    idx, dropped = score.resolve_genes(None, [4, 2], 5)
    assert idx.tolist() == [4, 2] and dropped == []
    with pytest.raises(ValueError):
        score.resolve_genes(None, ["PCNA"], 5)
    with pytest.raises(ValueError):
        score.resolve_genes(names, np.array([True, False]), 5)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def test_reference_scores_the_known_answer():
    csr = S.Csr.from_rows(KAT["n_genes"], [[(g, float(v)) for g, v in r] for r in KAT["rows"]], np.float64)
    assert (csr.values == 0).sum() == 1 and (csr.values < 0).sum() == 1
    mean = csr.dense().sum(axis=0) / csr.n
    assert mean.tolist() == [float(m) for m in KAT["means"]]
    got, ctrl, scale = S.score(csr, mean, [KAT["sets"]["a"], KAT["sets"]["b"]], None, KAT["ctrl_size"], KAT["n_bins"])
    assert got[:, 0].tolist() == [float(v) for v in KAT["scores"]["a"]] and got[:, 1].tolist() == [float(v) for v in KAT["scores"]["b"]]
    assert scale == 62 - 5 - 1                                  # max_abs = 16 < 2^5, the longest list has 2 genes


def test_reference_fixed_point():
    assert S.scale_log2(0.0, 1) == 62 and S.scale_log2(1.0, 1) == 61 and S.scale_log2(0.99, 64) == 56 and S.scale_log2(2.0 ** -40, 65) == 62 + 30 - 7
    csr = S.Csr.from_rows(3, [[(0, 0.1), (1, 0.2), (2, 0.30000000000000004)], []], np.float64)
    SUM, cnt, s, Sint = S.list_sums(csr, [[0, 1, 2], [1]])
    from fractions import Fraction
    exact = Fraction(0.1) + Fraction(0.2) + Fraction(0.30000000000000004)
    assert cnt.tolist() == [[3, 1], [0, 0]] and s == 62 + 1 - 2
    assert abs(Fraction(Sint[0][0], 2 ** s) - exact) <= 3 * Fraction(1, 2 ** (s + 1))           # the definition's bound, on the integers
    assert abs(Fraction(float(SUM[0, 0])) - exact) <= 3 * Fraction(1, 2 ** (s + 1)) + Fraction(np.spacing(SUM[0, 0])) / 2      # f64(S_int) rounds
    assert Sint[0][1] == round(0.2 * 2 ** s) and SUM[1].tolist() == [0.0, 0.0]


# ---- the layers ------------------------------------------------------------------------------------------------------------------------------------
def test_score_symbols_are_exported_and_bound():
    from singlerust_amd import _abi, _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS and name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    for s in ("SrxGeneListInfo", "SrxScoreGenesOpts", "SrxScoreGenesInfo"):
        assert "pub struct %s" % s in rust, s
    for fn in ("gene_list_sums", "score_genes", "score_genes_cell_cycle", "qc_gene_fractions", "score_genes_controls", "cell_cycle_phase"):
        assert callable(getattr(processing, fn)), fn
    for fn in ("gene_list_sums", "score_genes", "score_genes_cell_cycle", "qc_gene_fractions"):
        assert re.search(r"pub fn %s\b" % fn, shim), fn
        assert re.search(r"\b%s\(" % fn, mirror), fn
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header) and re.search(r"#define\s+SRX_GENE_LISTS_MAX\s+4096\b", header)
    assert "gene_sets.hip" in build.SOURCES
    for word in ("scanpy", "use_raw", "weighted signatures", "ties to even"):
        assert word in header.split("sums over gene lists per cell")[1].split("#define SRX_GENE_LISTS_MAX")[0], word


@pytest.mark.parametrize("cname,struct,size", [("srx_gene_list_info", "GeneListInfo", 64), ("srx_score_genes_opts", "ScoreGenesOpts", 24),
                                                ("srx_score_genes_info", "ScoreGenesInfo", 96)])
def test_score_struct_layout_matches_header(tmp_path, cname, struct, size):
    st = getattr(F(), struct)
    fields = [n for n, _ in st._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "srx.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
            + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(st)] + [getattr(st, f).offset for f in fields]
    assert C.sizeof(st) == size


def test_null_handles_are_refused_and_nothing_is_written():
    f = F()
    lib = f.lib()
    ptr, genes = np.array([0, 1], dtype=np.uint64), np.array([0], dtype=np.uint64)
    out, cnt = np.full(4, -7.0), np.full(4, 7, dtype=np.uint32)
    gi, si = f.GeneListInfo(), f.ScoreGenesInfo()
    gi.max_abs = si.max_abs = -7.0
    assert lib.srx_gene_list_sums(None, f.ptr(ptr), f.ptr(genes), 1, f.ptr(out), f.ptr(cnt), C.byref(gi)) == f.E_ARG
    assert b"null matrix" in lib.srx_last_error(None)
    assert lib.srx_score_genes(None, f.ptr(ptr), f.ptr(genes), 1, None, 0, None, f.ptr(out), None, None, 0, C.byref(si)) == f.E_ARG
    assert np.all(out == -7.0) and np.all(cnt == 7) and gi.max_abs == -7.0 and si.max_abs == -7.0


def test_gene_sets_source_has_no_floating_point_atomic_and_no_contraction():
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "gene_sets.hip")).read()
    assert "fp contract(off)" in src and '#include "hash.hpp"' in src and re.search(r"(?<!\w)value_scan\(m, ", src)
    assert not re.search(r"unsafeAtomicAdd|__hip_atomic|atomicExch|atomicCAS|atomicMax|atomicMin", src)
    targets = re.findall(r"atomicAdd\(&(\w+)\[", src)
    assert sorted(set(targets)) == ["my_cnt", "my_sum"]                       # the integer accumulators in LDS, nothing else
    assert re.search(r"unsigned long long\* my_sum", src) and re.search(r"uint32_t\* my_cnt", src)
    assert "mix64(" in src and not re.search(r"0xBF58476D1CE4E5B9", src)      # the hash is hash.hpp's, stated once


def test_gene_set_kernels_do_not_spill_registers(tmp_path):
    from singlerust_amd import build
    out = str(tmp_path / "gene_sets.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "gene_sets.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S*k_gs_\S*)\n(.*?)\.wavefront_size", text, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen += 1
    assert seen == 9                                             # the walk at 2 index widths x 2 storages x 2 bitmap places, and the score
