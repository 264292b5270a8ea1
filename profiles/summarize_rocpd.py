#!/usr/bin/env python3
"""Kernel-stats table (calls / total / avg / min / max, VGPRs, LDS) from a rocprofv3 rocpd
database (`rocprofv3 --kernel-trace --stats -d DIR -o NAME -- cmd` writes NAME_results.db).
Usage: python profiles/summarize_rocpd.py DIR/x_results.db [--last N] > profiles/rNN_x.md
--last N: only the last N dispatches of every kernel (the timed calls at the end of a script that ran others before them)."""
import sqlite3
import sys


def main(path, last=0):
    c = sqlite3.connect(path)
    tables = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tables if "kernel_dispatch" in t][0]
    ks = [t for t in tables if "kernel_symbol" in t][0]
    src = kd if not last else (f"(select *, row_number() over (partition by kernel_id order by start desc) as back_ from {kd})")
    where = "" if not last else f"where d.back_ <= {int(last)}"
    rows = c.execute(f"""
        select s.display_name, count(*), sum(d.end - d.start), avg(d.end - d.start), min(d.end - d.start),
               max(d.end - d.start), s.arch_vgpr_count, s.sgpr_count, max(d.group_segment_size),
               max(d.private_segment_size), max(d.grid_size_x), max(d.workgroup_size_x)
        from {src} d join {ks} s on d.kernel_id = s.id {where} group by s.display_name order by 3 desc""").fetchall()
    total = sum(r[2] for r in rows) or 1
    print("| kernel | calls | total ms | avg us | min us | max us | % | vgpr | sgpr | lds B | scratch B | grid | wg |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        name = r[0].replace("|", "\\|")
        if len(name) > 90:
            name = name[:87] + "..."
        print(f"| `{name}` | {r[1]} | {r[2] / 1e6:.3f} | {r[3] / 1e3:.1f} | {r[4] / 1e3:.1f} | {r[5] / 1e3:.1f} | "
              f"{100 * r[2] / total:.1f} | {r[6]} | {r[7]} | {r[8]} | {r[9]} | {r[10]} | {r[11]} |")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[sys.argv.index("--last") + 1]) if "--last" in sys.argv else 0)
