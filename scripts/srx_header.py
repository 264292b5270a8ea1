"""Parse the C ABI headers (include/srx.h, include/srx_synth.h) into plain data, all of it in C terms: C type strings and
declarator names.  The two binding generators render it: scripts/gen_rust_bindings.py (rust/srx_sys.rs) and
scripts/gen_ctypes_bindings.py (singlerust_amd/_abi.py).

This is not a C parser.  It reads the subset the headers are written in: `#define SRX_X <integer>`, named and anonymous
enums, `typedef struct X X;` (opaque handles), `typedef struct X {...} X;` with scalar, pointer, array and
multi-declarator fields, one style of function-pointer typedef, and prototypes of `srx_*` functions.  Anything else
fails an assertion here or an "unknown C type" in a renderer, so a header that outgrows it is noticed at generation.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRX_H = os.path.join(ROOT, "include", "srx.h")
SRX_SYNTH_H = os.path.join(ROOT, "include", "srx_synth.h")

Decl = tuple[str, str]                       # (C type, declarator name): ('const uint64_t*', 'sel')


@dataclass
class Header:
    consts: list[tuple[str, int]] = field(default_factory=list)       # every #define, then every enum member
    enums: dict[str, list[tuple[str, int]]] = field(default_factory=dict)             # the named enums and their members
    opaque: list[str] = field(default_factory=list)                   # typedef struct X X;
    structs: dict[str, list[tuple[str, str, str | None]]] = field(default_factory=dict)   # (C type, name, array length)
    fnptrs: dict[str, tuple[str, list[Decl]]] = field(default_factory=dict)           # name -> (return type, parameters)
    funcs: list[tuple[str, str, list[Decl]]] = field(default_factory=list)            # (name, return type, parameters)


def split_type(ctype: str) -> tuple[str, int, bool]:
    """'const srx_mat**' -> ('srx_mat', 2, True): the base type's name, the pointer depth, whether `const` occurs."""
    words = ctype.replace("*", " ").split()
    base = [w for w in words if w not in ("const", "struct", "enum")]
    assert len(base) == 1, ctype
    return base[0], ctype.count("*"), "const" in words


def strip_comments(src: str) -> str:
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)            # preprocessor lines
    src = re.sub(r'extern\s+"C"\s*\{', " ", src)
    return src


def split_decl(decl: str) -> tuple[str, str, str | None]:
    """'const uint64_t* sel' -> ('const uint64_t*', 'sel', None);  'double v[SRX_N]' -> ('double', 'v', 'SRX_N')"""
    m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[([^\]]*)\])?$", decl.strip(), flags=re.S)
    assert m, decl
    return " ".join(m.group(1).split()), m.group(2), m.group(3).strip() if m.group(3) else None


def _params(text: str) -> list[Decl]:
    text = " ".join(text.split())
    if not text or text == "void":
        return []
    out = []
    for p in text.split(","):
        ctype, name, arr = split_decl(p)
        assert ctype and arr is None, p
        out.append((ctype, name))
    return out


def parse(*paths: str) -> Header:
    """Parse the headers as one text, in the order given: srx_synth.h uses the opaque handles srx.h declares."""
    raw = "\n".join(open(p).read() for p in paths)
    h = Header()
    for m in re.finditer(r"#define\s+(SRX_[A-Z0-9_]+)\s+(\d+)", raw):
        h.consts.append((m.group(1), int(m.group(2))))
    src = strip_comments(raw)
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", src):
        h.opaque.append(m.group(2))
    enum_re = r"(?:typedef\s+)?enum\s*(\w*)\s*\{(.*?)\}\s*(\w*)\s*;"
    for m in re.finditer(enum_re, src, flags=re.S):
        members, nxt = [], 0
        for item in m.group(2).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                item, v = (s.strip() for s in item.split("="))
                nxt = int(v, 0)
            members.append((item, nxt))
            nxt += 1
        h.consts += members
        if m.group(3):
            h.enums[m.group(3)] = members
    src = re.sub(enum_re, " ", src, flags=re.S)
    for m in re.finditer(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\((.*?)\)\s*;", src, flags=re.S):
        h.fnptrs[m.group(2)] = (m.group(1), _params(m.group(3)))
    struct_re = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;"
    for m in re.finditer(struct_re, src, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            if not stmt.strip():
                continue
            # `uint64_t a, b, c` -> three fields of the same type
            first, *rest = stmt.split(",")
            ctype, name, arr = split_decl(first)
            assert ctype, stmt
            fields.append((ctype, name, arr))
            for d in rest:
                none, name, arr = split_decl(d)
                assert not none, stmt                            # `T a, *b` is not written in these headers
                fields.append((ctype, name, arr))
        h.structs[m.group(3)] = fields
    src = re.sub(struct_re, " ", src, flags=re.S)
    src = re.sub(r"typedef[^;]*;", " ", src)
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(srx_\w+)\s*\(([^()]*)\)\s*;", src, flags=re.S):
        h.funcs.append((m.group(2), " ".join(m.group(1).split()), _params(m.group(3))))
    return h
