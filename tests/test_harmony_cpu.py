"""The numpy restatement of the Harmony definition (tests/harmony_ref.py) is the yardstick of the device tests, so it is
tested itself: the closed-form correction against a dense solve, the invariants of R, O and E, the one-batch identity, and
what the method is for (batches mix, cell types stay apart) on two planted data sets."""
import numpy as np
import pytest

import harmony_ref as ref

_RUN = {}


def run_planted(name):
    if name not in _RUN:
        Z, batch, typ = ref.planted_two() if name == "two" else ref.planted_seven()
        B, K = (2, 20) if name == "two" else (7, 65)
        _RUN[name] = (Z, batch, typ, ref.run(Z, batch, B, n_clusters=K))
    return _RUN[name]


def test_closed_form_correction_equals_the_dense_ridge_solve():
    rng = np.random.default_rng(0)
    K, B, d = 5, 6, 4
    m = rng.uniform(0.1, 30.0, (K, B))
    m[:, 3] = 0.0                                     # an empty batch
    S = rng.normal(0, 5, (K, B, d)) * m[:, :, None]
    for lam in (1.0, 0.25, 7.0):
        W = ref.ridge_closed_form(m, S, lam)
        for k in range(K):
            dense = ref.ridge_dense(m[k], S[k], lam)
            assert np.abs(W[k] - dense).max() <= 1e-12 * max(1.0, np.abs(dense).max())
        assert np.all(W[:, 3] == 0)


def test_one_batch_returns_the_input():
    Z, batch, _ = ref.planted_two()
    out = ref.run(Z, np.zeros_like(batch), 1, n_clusters=20)
    assert np.abs(out["Z_corr"] - Z).max() <= 1e-12 * np.abs(Z).max()


@pytest.mark.parametrize("name", ["two", "seven"])
def test_R_O_E_invariants(name):
    Z, batch, _, out = run_planted(name)
    R, O, E = out["R"], out["O"], out["E"]
    n, B = Z.shape[0], O.shape[1]
    assert np.abs(R.sum(axis=1) - 1).max() < 1e-12
    assert np.abs(O.sum(axis=1) - R.sum(axis=0)).max() < 1e-10 * n
    onehot = np.zeros((n, B))
    onehot[np.arange(n), batch] = 1
    O2 = ref.tables(R, onehot)
    E2 = np.outer(R.sum(axis=0), np.bincount(batch, minlength=B) / n)
    assert np.abs(O2 - O).max() <= 1e-10 * max(1.0, np.abs(O2).max())
    assert np.abs(E2 - E).max() <= 1e-10 * max(1.0, np.abs(E2).max())


def test_planted_two_batches_mix_and_types_stay():
    Z, batch, typ, out = run_planted("two")
    before, _ = ref.mixing_and_purity(Z, batch, typ)
    after, purity = ref.mixing_and_purity(out["Z_corr"], batch, typ)
    print("mixing", before, after, "purity", purity, "rounds", out["rounds"], out["round_iters"])
    assert before < 0.15 and after > 0.4 and purity >= 0.99
    assert out["converged"] == 1 and out["rounds"] <= 10


def test_planted_seven_batches_with_an_empty_one():
    Z, batch, typ, out = run_planted("seven")
    assert not np.any(batch == 5)
    before, _ = ref.mixing_and_purity(Z, batch, typ)
    after, purity = ref.mixing_and_purity(out["Z_corr"], batch, typ)
    print("mixing", before, after, "purity", purity, "rounds", out["rounds"], out["round_iters"])
    assert after > before and purity >= 0.99
    assert np.all(out["O"][:, 5] == 0) and np.all(out["E"][:, 5] == 0)
    assert out["converged"] == 1


def test_stopping_ratios_are_clear_of_their_epsilons():
    for name in ("two", "seven"):
        out = run_planted(name)[3]
        assert all(abs(r - 1e-5) >= 1e-9 for r in out["ratios_cluster"])
        assert all(abs(r - 1e-4) >= 1e-9 for r in out["ratios_harmony"])


def test_hashes_and_defaults():
    # splitmix64 of the UMAP section: mix(seed + G) for seed 0 is the generator's first output
    assert int(ref.mix(np.array([ref.GOLD], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert int(ref.hashes(0, 0, 3)[0]) == 0xE220A8397B1DCDAF
    assert [ref.default_clusters(n) for n in (1, 14, 15, 44, 45, 600, 3000, 10 ** 6)] == [1, 1, 1, 1, 2, 20, 100, 100]


def test_float_type_switch_agrees():
    Z, batch, _ = ref.planted(120, 6, 3, 3, 5)
    kw = dict(n_clusters=7, epsilon_cluster=0.0, epsilon_harmony=0.0, max_rounds=2, max_cluster_iters=3)
    a = ref.run(Z, batch, 3, **kw)
    b = ref.run(Z, batch, 3, ft=np.longdouble, **kw)
    g = ref.gaps(a, b)
    print(g)
    assert b["R"].dtype == np.longdouble and max(g.values()) < 1e-12
