"""srx_louvain_csr against the definition of include/srx.h, decision for decision.  On the cases of louvain_ref.EXACT_RUNS every
weight is a multiple of 2^-20 and 2m < 2^32 (tests/test_louvain_cpu.py asserts it), so k_i, tot_c, w_{i->c} and every coarse
weight are exact in f64 and in the device's fixed point, g(c) = w_to - gamma * ki * t / twom sees the same bits on both sides,
and every comparison and every tie falls the same way: labels, sweeps, moves and the communities of every level are EQUAL to
the host restatement's.  Only Q, which the device makes from fixed-point sums, is held to 1e-9; no keep-or-discard decision of
these cases is closer than 1e-8 (asserted there too).

The resident route (srx_louvain on a graph handle) is not run here: a handle is only made from points or from a k-NN list,
through real-valued recomputation, never from a caller's CSR.  tests/test_louvain_gpu.py holds it equal to srx_louvain_csr."""
import json

import numpy as np
import pytest

import louvain_ref as ref
from test_louvain_gpu import check_invariants, run

pytestmark = pytest.mark.gpu

COUNTS = ("n_communities", "n_levels", "sweeps", "moves", "level_communities")


def device(ctx, W, opts):
    kw = dict(opts)
    if "gamma" in kw:
        kw["resolution"] = kw.pop("gamma")
    return run(ctx, W, **kw)


def _localise(ctx, W, opts, got, want):
    """Where the two sides part: the first level whose community count differs and, within the first level, the first sweep
    after which the partitions differ, with a vertex on which they do."""
    lines = ["%s: device %s, restatement %s" % (k, got[1][k], want[1][k]) for k in COUNTS if got[1][k] != want[1][k]]
    if not np.array_equal(got[0], want[0]):
        lines.append("labels differ on %d of %d vertices" % (int((got[0] != want[0]).sum()), len(want[0])))
    a, b = got[1]["level_communities"], want[1]["level_communities"]
    level = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    lines.append("first level with another community count: %d (of %d on the device, %d in the restatement)" % (level + 1, len(a), len(b)))
    base = {k: v for k, v in opts.items() if k in ("gamma", "max_sweeps")}
    one = dict(base, max_levels=1)
    if np.array_equal(device(ctx, W, one)[0], ref.louvain(W, **one)[0]):
        lines.append("the first level alone agrees")
        return "\n".join(lines)
    lens = np.diff(W.indptr)
    for sweeps in range(1, 17):
        pre = dict(one, max_sweeps=sweeps)
        d, r = device(ctx, W, pre)[0], ref.louvain(W, **pre)[0]
        if not np.array_equal(d, r):
            coo = W.tocoo()                      # an edge that one side has inside a community and the other has not
            e = np.flatnonzero((d[coo.row] == d[coo.col]) != (r[coo.row] == r[coo.col]))
            v, u = (int(coo.row[e[0]]), int(coo.col[e[0]])) if len(e) else (int(np.flatnonzero(d != r)[0]), -1)
            lines.append("the first level differs after sweep %d (parity %d): vertex %d, a row of %d entries, shares its community "
                         "with its neighbour %d on %s only" % (sweeps, (sweeps - 1) & 1, v, lens[v], u,
                                                                "the device" if d[v] == d[u] else "the restatement"))
            return "\n".join(lines)
    lines.append("the first level agrees through 16 sweeps and differs later")
    return "\n".join(lines)


def compare(ctx, name, opts):
    W = ref.exact_graph(name)
    want = ref.exact_result(name, opts)
    got = device(ctx, W, opts)
    print(json.dumps({"case": ref.run_id((name, opts)), "n": W.shape[0], "nnz": int(W.nnz), "ms": got[1]["ms"],
                      "levels": got[1]["level_communities"], "sweeps": got[1]["sweeps"], "moves": got[1]["moves"],
                      "restatement_level_sweeps": want[1]["level_sweeps"]}))
    if not (np.array_equal(got[0], want[0]) and all(got[1][k] == want[1][k] for k in COUNTS)):
        pytest.fail(ref.run_id((name, opts)) + "\n" + _localise(ctx, W, opts, got, want))
    lm_dev, lm_ref = got[1]["level_modularity"], want[1]["level_modularity"]
    assert len(lm_dev) == len(lm_ref) and all(abs(a - b) <= 1e-9 for a, b in zip(lm_dev, lm_ref)), (lm_dev, lm_ref)
    assert abs(got[1]["modularity"] - want[1]["modularity"]) <= 1e-9
    check_invariants(ctx, W, got[0], got[1], gamma=opts.get("gamma", 1.0), first_level=False)
    return got


@pytest.mark.parametrize("run_", ref.EXACT_RUNS, ids=ref.run_id)
def test_equal_to_the_restatement(ctx, run_):
    compare(ctx, *run_)


@pytest.mark.parametrize("run_", ref.prefix_runs(), ids=ref.run_id)
def test_first_level_sweep_prefixes(ctx, run_):
    """max_sweeps ends a level with the labelling the last sweep left; sweeps 1 and 2 move the two parities."""
    got = compare(ctx, *run_)
    assert got[1]["sweeps"] == run_[1]["max_sweeps"] and got[1]["n_levels"] == 1


@pytest.mark.parametrize("run_", ref.guard_runs(), ids=ref.run_id)
def test_guard_cases_by_hand(ctx, run_):
    """Against the labels written out by hand (traces in tests/test_louvain_cpu.py), so that an error the restatement shared
    would fail too; then against the restatement."""
    name, opts, want = run_
    labels, info = device(ctx, ref.exact_graph(name), opts)
    assert np.array_equal(labels, want), (labels, want)
    compare(ctx, name, opts)
