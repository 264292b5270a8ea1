#!/usr/bin/env python3
"""Generate singlerust_amd/_abi.py — the ctypes description of libsrx_hip.so's C ABI (constants, structures, the
signature of every function) — from include/srx.h and include/srx_synth.h, so that the Python binding cannot drift
from the headers.  singlerust_amd/_ffi.py loads the library and applies the generated SIGNATURES.

What is checked (tests/test_abi_cpu.py): the committed file is exactly what this script produces from the current
headers; every structure has the size, field offsets and field sizes the C compiler gives it; the functions are the
ones the headers declare and the library exports, each with its arity.

    python scripts/gen_ctypes_bindings.py            # rewrite singlerust_amd/_abi.py
    python scripts/gen_ctypes_bindings.py --check    # exit 1 if the committed file is stale

The mapping.  `SRX_X` (a #define or an enum member) -> `X`; `srx_foo_bar` -> `class FooBar`; fields keep their header
names (a Python keyword gets a trailing underscore); scalars and enums by value -> the exact-width ctypes type;
`const char*` returned -> c_char_p; a struct by value -> its class; `struct*` -> POINTER(Class); any `T**` ->
POINTER(c_void_p); every other pointer (handles, scalar arrays, out-scalars, a callback) -> c_void_p, which takes
`byref(x)`, an array, `_ffi.ptr(a)` or None.  Only inside the callback typedef is a scalar pointer POINTER(scalar): the
Python callback reads through it.
"""
from __future__ import annotations

import keyword
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srx_header  # noqa: E402

OUT = os.path.join(srx_header.ROOT, "singlerust_amd", "_abi.py")

SCALARS = {
    "int8_t": "C.c_int8", "uint8_t": "C.c_uint8", "int16_t": "C.c_int16", "uint16_t": "C.c_uint16", "int32_t": "C.c_int32",
    "uint32_t": "C.c_uint32", "int64_t": "C.c_int64", "uint64_t": "C.c_uint64", "size_t": "C.c_size_t", "double": "C.c_double",
    "float": "C.c_float", "char": "C.c_char", "int": "C.c_int",
}
WIDTH = 118


def const_name(name: str) -> str:
    assert name.startswith("SRX_"), name
    return name[4:]


def class_name(name: str) -> str:
    assert name.startswith("srx_"), name
    return "".join(p.capitalize() for p in name[4:].split("_"))


def ident(name: str) -> str:
    return name + "_" if keyword.iskeyword(name) else name


class Types:
    def __init__(self, header: srx_header.Header):
        self.h = header

    def ctypes(self, ctype: str, typed_scalar_pointers: bool = False) -> str:
        """C type of a field, a parameter or a return value -> the ctypes expression."""
        b, n_ptr, _ = srx_header.split_type(ctype)
        known = b == "void" or b in SCALARS or b in self.h.enums or b in self.h.structs or b in self.h.opaque or b in self.h.fnptrs
        if not known or (b == "void" and n_ptr == 0):
            raise ValueError(f"unknown C type {ctype!r}")
        if n_ptr == 0:
            if b in self.h.fnptrs:
                return "P"
            if b in self.h.structs:
                return class_name(b)
            return "C.c_int32" if b in self.h.enums else SCALARS[b]          # C enums cross the ABI as int
        if n_ptr >= 2:
            return "C.POINTER(P)"
        if b in self.h.structs:
            return f"C.POINTER({class_name(b)})"
        if typed_scalar_pointers and b in SCALARS:
            return f"C.POINTER({SCALARS[b]})"
        return "P"

    def restype(self, ctype: str) -> str:
        if ctype == "void":
            return "None"
        return "C.c_char_p" if ctype.replace(" ", "") == "constchar*" else self.ctypes(ctype)


def wrap(head: str, items: list[str], tail: str) -> list[str]:
    """`head` + the items, comma-separated, + `tail`, broken before WIDTH columns with continuation lines aligned behind `head`."""
    lines, cur = [], head
    for i, it in enumerate(items):
        piece = it + (", " if i + 1 < len(items) else "")
        if len(cur) + len(piece.rstrip()) > WIDTH and cur.strip() and cur != head:
            lines.append(cur.rstrip())
            cur = " " * len(head)
        cur += piece
    lines.append(cur + tail)
    return lines


def render() -> str:
    h = srx_header.parse(srx_header.SRX_H, srx_header.SRX_SYNTH_H)
    ty = Types(h)
    consts = dict(h.consts)
    o = ['"""singlerust_amd/_abi.py — GENERATED from include/srx.h and include/srx_synth.h by scripts/gen_ctypes_bindings.py;',
         "do not edit.  The ctypes description of libsrx_hip.so's C ABI: constants, structures, the signature of every function.",
         "To change it, edit the header and run the generator (and scripts/gen_rust_bindings.py).  singlerust_amd/_ffi.py loads",
         'the library and applies SIGNATURES."""',
         "import ctypes as C",
         "",
         "P = C.c_void_p",
         ""]
    for k, v in h.consts:
        o.append(f"{const_name(k)} = {v}")
    o.append("")
    o += wrap("STATUS_NAMES = {", [f'{v}: "{k}"' for k, v in h.enums["srx_status"]], "}")
    for name, fields in h.structs.items():
        o += ["", ""]
        o.append(f"class {class_name(name)}(C.Structure):      # {name}")
        items = []
        for ctype, fname, arr in fields:
            t = ty.ctypes(ctype)
            items.append(f'("{ident(fname)}", {t} * {consts[arr] if arr in consts else int(arr)})' if arr else f'("{ident(fname)}", {t})')
        o += wrap("    _fields_ = [", items, "]")
    o += ["", ""]
    for name, (ret, params) in h.fnptrs.items():
        args = [ty.restype(ret)] + [ty.ctypes(t, typed_scalar_pointers=True) for t, _ in params]
        o += wrap(f"{name[4:].upper()} = C.CFUNCTYPE(", args, f")      # {name}")
    o.append("")
    o.append("SIGNATURES = {")
    o.append("    # name: (restype, argtypes)")
    for name, ret, params in h.funcs:
        o += wrap(f'    "{name}": ({ty.restype(ret)}, [', [ty.ctypes(t) for t, _ in params], "]),")
    o.append("}")
    o.append("EXPORTS = tuple(SIGNATURES)")
    o.append("")
    return "\n".join(o)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == text
        print("singlerust_amd/_abi.py is", "up to date" if ok else "STALE: run scripts/gen_ctypes_bindings.py")
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        f.write(text)
    n_funcs = text.count('\n    "srx_')
    print(f"wrote {OUT}: {text.count('(C.Structure)')} structures, {n_funcs} functions")
