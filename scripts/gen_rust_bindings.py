#!/usr/bin/env python3
"""Generate rust/srx_sys.rs — the `extern "C"` module a SingleRust maintainer adds — from
include/srx.h, so that the Rust declarations cannot drift from the C ABI.

The image has no rustc: the output is NOT compile-checked.  What is checked (tests/test_abi_cpu.py) is that the
committed file is exactly what this script produces from the current header, and that it declares every function
the shared library exports for include/srx.h.

    python scripts/gen_rust_bindings.py            # rewrite rust/srx_sys.rs
    python scripts/gen_rust_bindings.py --check    # exit 1 if the committed file is stale
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srx_header  # noqa: E402

ROOT = srx_header.ROOT
OUT = os.path.join(ROOT, "rust", "srx_sys.rs")

SCALARS = {
    "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "size_t": "usize", "double": "f64",
    "float": "f32", "uint8_t": "u8", "int8_t": "i8", "uint16_t": "u16", "int16_t": "i16", "char": "c_char", "int": "i32",
}
RUST_KEYWORDS = {"type", "fn", "in", "ref", "mod", "use", "box", "loop", "match", "move", "self", "super", "where"}


def camel(name: str) -> str:
    return "".join(p.capitalize() for p in name.split("_"))


class Types:
    def __init__(self, header: srx_header.Header):
        self.h = header

    def rust(self, ctype: str) -> str:
        """C type (no declarator name) -> Rust type."""
        b, n_ptr, const = srx_header.split_type(ctype)
        if b in self.h.fnptrs and n_ptr == 0:
            return camel(b)                                      # the `pub type` alias below
        if b == "void":
            r = "c_void"
            assert n_ptr >= 1, ctype
        elif b in SCALARS:
            r = SCALARS[b]
        elif b in self.h.enums:
            r = "i32"                                            # C enums cross the ABI as int
        elif b in self.h.structs or b in self.h.opaque:
            r = camel(b)
        else:
            raise ValueError(f"unknown C type {ctype!r}")
        for i in range(n_ptr):
            # `const T*` -> *const T; the const binds to the pointee of the innermost pointer only
            r = ("*const " if (const and i == 0) else "*mut ") + r
        return r

    def args(self, params) -> str:
        return ", ".join(f"{ident(n)}: {self.rust(t)}" for t, n in params)


def ident(name: str) -> str:
    name = name.rstrip("_") if name.endswith("_") and name[:-1] not in RUST_KEYWORDS else name
    return name + "_" if name in RUST_KEYWORDS else name


def render() -> str:
    h = srx_header.parse(srx_header.SRX_H)
    ty = Types(h)
    o = []
    o.append("// rust/srx_sys.rs — GENERATED from include/srx.h by scripts/gen_rust_bindings.py; do not edit.")
    o.append("// `extern \"C\"` declarations of libsrx_hip.so for the shim of INTEGRATION.md (src/gpu/ffi.rs in a SingleRust")
    o.append("// checkout, behind a cargo feature).  Not compile-checked here: the build image has no rustc.  The hand-written")
    o.append("// part of the binding (the `upload` helper and the replaced function bodies) is rust/shim.rs.")
    o.append("#![allow(non_camel_case_types, dead_code)]")
    o.append("use std::os::raw::{c_char, c_void};")
    o.append("")
    for k, v in h.consts:
        t = "usize" if k in ("SRX_UNIQUE_ID_BYTES",) else "i32"
        # rustc denies an out-of-range literal (overflowing_literals): one such constant and the whole module fails to compile
        assert t != "i32" or -2**31 <= v < 2**31, f"{k} = {v} does not fit the i32 it is rendered as"
        o.append(f"pub const {k}: {t} = {v};")
    o.append("")
    for name in h.opaque:
        if name in h.structs:
            continue
        o.append(f"#[repr(C)] pub struct {camel(name)} {{ _private: [u8; 0] }}      // opaque `{name}`")
    o.append("")
    for name, fields in h.structs.items():
        o.append("#[repr(C)]")
        o.append("#[derive(Clone, Copy)]")
        o.append(f"pub struct {camel(name)} {{      // `{name}`")
        for ctype, fname, arr in fields:
            ftype = f"[{ty.rust(ctype)}; {arr} as usize]" if arr else ty.rust(ctype)
            o.append(f"    pub {ident(fname)}: {ftype},")
        o.append("}")
        o.append("")
    for name, (ret, params) in h.fnptrs.items():
        o.append(f"pub type {camel(name)} = extern \"C\" fn({ty.args(params)}) -> {ty.rust(ret)};      // `{name}`")
    o.append("")
    o.append('#[link(name = "srx_hip")]')
    o.append('extern "C" {')
    for name, ret, params in h.funcs:
        args = [(ident(n), ty.rust(t)) for t, n in params]
        ret = None if ret == "void" else ty.rust(ret)
        a = ", ".join(f"{n}: {t}" for n, t in args)
        line = f"    pub fn {name}({a})" + (f" -> {ret}" if ret else "") + ";"
        if len(line) > 118:
            pad = " " * (len(f"    pub fn {name}("))
            chunks, cur = [], ""
            for i, (n, t) in enumerate(args):
                piece = f"{n}: {t}" + (", " if i + 1 < len(args) else "")
                if len(pad) + len(cur) + len(piece) > 116 and cur:
                    chunks.append(cur.rstrip())
                    cur = ""
                cur += piece
            chunks.append(cur)
            line = f"    pub fn {name}(" + ("\n" + pad).join(chunks) + ")" + (f" -> {ret}" if ret else "") + ";"
        o.append(line)
    o.append("}")
    o.append("")
    return "\n".join(o)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == text
        print("rust/srx_sys.rs is", "up to date" if ok else "STALE: run scripts/gen_rust_bindings.py")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: {text.count('pub fn ')} functions")
