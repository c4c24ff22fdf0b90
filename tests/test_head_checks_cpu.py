"""No GPU: the comparators of tests/util_head.py bite, and the case tables of tests/test_head_paths_gpu.py are sound.

Each mutant below is a structural mistake a head kernel could make, applied in numpy to the float64 oracle's result.
The comparator must reject it, and must accept the unmutated float32 oracle on the same case -- so the margin is
checkable without a device."""
import numpy as np
import pytest

from oracle import head_oracle as ho
from tests import util_head as uh

D0 = (1024, 18, 3)


def rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def accepts_float32_oracle(case, quantities):
    for q in quantities:
        uh.assert_close(getattr(case.ref(np.float32), q), case, q)


# ---- the mutants ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [33, 512, 2100])
def test_mutant_dw1_forgets_the_last_batch_row(B):
    case = uh.Case(*D0, B)
    r = case.ref()
    mutant = r.dW1 - np.outer(case.x[-1].astype(np.float64), r.dpre[-1])
    dev = uh.deviation(mutant, r.dW1) / np.abs(r.dW1).max()
    assert dev > 1e4 * uh.roundoff_unit(case, "dW1") and dev > 1e-2
    assert rejected(uh.assert_close, mutant, case, "dW1")
    assert rejected(uh.assert_close, mutant, case, "dW1", margin=10 * uh.margin_for(case, "dW1"))
    accepts_float32_oracle(case, uh.BLOCKS)


@pytest.mark.parametrize("B", [65, 511, 2100])
def test_mutant_dw1_forgets_the_last_row_of_one_slice(B):
    case = uh.Case(*D0, B)
    r = case.ref()
    rows_per = -(-B // 32)
    row = 4 * rows_per - 1                                      # last row of slice 3
    mutant = r.dW1 - np.outer(case.x[row].astype(np.float64), r.dpre[row])
    assert uh.deviation(mutant, r.dW1) / np.abs(r.dW1).max() > 1e4 * uh.roundoff_unit(case, "dW1")
    assert rejected(uh.assert_close, mutant, case, "dW1", margin=10 * uh.margin_for(case, "dW1"))
    accepts_float32_oracle(case, ("dW1",))


@pytest.mark.parametrize("regime", ["ordinary", "loud", "saturated"])
@pytest.mark.parametrize("in_dim,wave", [(1024, 2), (192, 3), (208, 3), (1040, 0), (80, 1)])
def test_mutant_forward_skips_the_last_chunk_of_a_wave(in_dim, wave, regime):
    dims = (in_dim, 18, 3)
    case = uh.forward_case(dims, regime)
    chunk = uh.mfma_wave_chunks(in_dim, wave)[-1]
    x = case.x.copy()
    x[:, 16 * chunk:16 * chunk + 16] = 0.0                      # the same as leaving the chunk out of the sum
    mutant, _ = ho.forward(case.p, x, *dims)
    assert uh.deviation(mutant, case.ref().probs) > 1e4 * uh.roundoff_unit(case, "probs")
    assert rejected(uh.assert_close, mutant, case, "probs", margin=10 * uh.margin_for(case, "probs"))
    assert rejected(uh.check_probs, mutant.astype(np.float32), case)
    uh.check_probs(case.ref(np.float32).probs, case)


@pytest.mark.parametrize("regime", ["ordinary", "loud", "saturated"])
def test_mutant_hidden_units_16_and_17_exchanged(regime):
    case = uh.forward_case(D0, regime)
    W1, b1, W2, b2 = [a.astype(np.float64) for a in ho.unpack(case.p, *D0)]
    h = case.ref().h.copy()
    h[:, [16, 17]] = h[:, [17, 16]]
    z = h @ W2 + b2
    e = np.exp(z - z.max(axis=1, keepdims=True))
    mutant = e / e.sum(axis=1, keepdims=True)
    assert rejected(uh.assert_close, mutant, case, "probs", margin=10 * uh.margin_for(case, "probs"))
    uh.check_probs(case.ref(np.float32).probs, case)


@pytest.mark.parametrize("dims", uh.REGIME_DIMS)
def test_mutant_loss_through_float32_log_of_p(dims):
    case = uh.Case(*dims, 257, "saturated")
    r32, r64 = case.ref(np.float32), case.ref()
    assert np.isinf(r32.loss_sum_via_log) and np.isfinite(r64.loss_sum_via_log)       # what the issue found: -log(p) overflows
    assert rejected(uh.check_loss_sum, r32.loss_sum_via_log, case)
    uh.check_loss_sum(r32.loss_sum, case)                                             # the logit form in float32 is fine
    assert r64.loss_rows.max() > 50 and r64.probs.min() < 1e-45


@pytest.mark.parametrize("dims", uh.REGIME_DIMS)
def test_mutant_dpre_without_the_tanh_derivative_on_saturated_units(dims):
    case = uh.Case(*dims, 200, "saturated")
    r = case.ref()
    W1, b1, W2, b2 = [a.astype(np.float64) for a in ho.unpack(case.p, *dims)]
    pre = case.x.astype(np.float64) @ W1 + b1
    sat = np.abs(pre) > 9
    assert 0.2 < sat.mean() < 0.8
    dz = r.probs.copy()
    dz[np.arange(case.B), case.y] -= 1.0
    dz /= case.B
    dpre = np.where(sat, dz @ W2.T, r.dpre)
    for q, mutant in (("dW1", case.x.astype(np.float64).T @ dpre), ("db1", dpre.sum(0))):
        assert rejected(uh.assert_close, mutant, case, q, margin=10 * uh.margin_for(case, q)), q
    accepts_float32_oracle(case, uh.BLOCKS)


def test_mutant_ncorrect_off_by_one():
    case = uh.Case(*D0, 200)
    nc = case.ref().ncorrect
    uh.check_ncorrect(float(nc), case)
    assert rejected(uh.check_ncorrect, float(nc + 1), case) and rejected(uh.check_ncorrect, float(nc - 1), case)
    assert rejected(uh.check_ncorrect, nc + 0.5, case)


class TorchPlacementAdam(ho.KerasAdam):
    """eps inside the bias-corrected square root: theta -= lr * mhat / (sqrt(vhat) + eps)."""

    def step(self, p, g):
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mhat, vhat = self.m / (1.0 - self.b1 ** self.t), self.v / (1.0 - self.b2 ** self.t)
        return p - self.lr * mhat / (np.sqrt(vhat) + self.eps)


class UncorrectedAdam(ho.KerasAdam):
    def step(self, p, g):
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        return p - self.lr * self.m / (np.sqrt(self.v) + self.eps)


@pytest.mark.parametrize("steps", [1, uh.ADAM_STEPS])
@pytest.mark.parametrize("mutant_cls", [TorchPlacementAdam, UncorrectedAdam])
def test_mutant_adam(mutant_cls, steps):
    ac = uh.AdamCase("default", steps=steps)
    mutant = ac.trajectory(np.float64, mutant_cls)
    assert uh.deviation(mutant, ac.trajectory()) > 1e2 * ac.unit()
    assert rejected(ac.assert_close, mutant, margin=10 * uh.MARGIN["adam"])
    ac.assert_close(ac.trajectory(np.float32))
    # zero-gradient parameters never move, in either precision
    for dt in (np.float32, np.float64):
        assert np.array_equal(ac.trajectory(dt)[ac.untouched()], ac.p0.astype(dt)[ac.untouched()])


@pytest.mark.parametrize("B", [33, 2100])
def test_mutant_db2_over_whole_64_row_chunks_only(B):
    case = uh.Case(*D0, B)
    r = case.ref()
    dz = r.probs.copy()
    dz[np.arange(B), case.y] -= 1.0
    dz /= B
    assert np.allclose(dz.sum(0), r.db2, rtol=0, atol=1e-15)
    mutant = dz[:64 * (B // 64)].sum(0)
    assert uh.deviation(mutant, r.db2) / np.abs(r.db2).max() > 0.1
    assert rejected(uh.assert_close, mutant, case, "db2", margin=10 * uh.margin_for(case, "db2"))
    accepts_float32_oracle(case, ("db2",))


# ---- the yardsticks themselves -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime", ["ordinary", "loud", "saturated"])
def test_loss_from_logits_is_the_oracles_loss_in_float64(regime):
    for dims in uh.REGIME_DIMS:
        case = uh.Case(*dims, 257, regime)
        rows = uh.loss_from_logits(case.p, case.x, case.y, dims)
        probs, _ = ho.forward(case.p, case.x, *dims)
        with np.errstate(divide="ignore"):
            via_log = -np.log(probs[np.arange(case.B), case.y])
        both = np.isfinite(via_log) & np.isfinite(rows)
        assert both.mean() > 0.5
        assert np.abs(rows[both] - via_log[both]).max() <= 1e-12 * np.maximum(1.0, np.abs(via_log[both])).max()
        if both.all():
            _, _, _, lsum = ho.loss_and_grad(case.p, case.x, case.y, *dims)
            assert abs(rows.sum() - lsum) <= 1e-12 * max(1.0, lsum)


def test_margins():
    """4 unless measured otherwise on the device; every mutant above is rejected at ten times the margin in use."""
    assert all(v == 4.0 for v in uh.MARGIN.values())
    assert set(uh.MARGIN_SATURATED) <= set(uh.MARGIN) and all(4.0 < v < 100.0 for v in uh.MARGIN_SATURATED.values())
    sat, plain = uh.Case(16, 1, 2, 2, "saturated"), uh.Case(16, 1, 2, 2, "loud")
    assert uh.margin_for(sat, "probs") == uh.MARGIN_SATURATED["probs"] and uh.margin_for(plain, "probs") == 4.0 == uh.margin_for(sat, "db2")


def test_zeros_only_below_the_smallest_denormal():
    case = uh.Case(*D0, 257, "saturated")
    p32 = case.ref(np.float32).probs.copy()
    uh.check_probs(p32, case)
    below = np.where(case.ref().probs < 2.0 ** -149, 0.0, p32).astype(np.float32)      # an exp that truncates at the last denormal
    uh.check_probs(below, case)
    flushed = np.where(p32 < 1.2e-38, 0.0, p32).astype(np.float32)                     # a kernel that flushed denormals to zero
    assert (flushed != p32).any() and rejected(uh.check_probs, flushed, case)


def test_blocks_split():
    g = np.arange(uh.nparams(5, 3, 2), dtype=np.float64)
    b = uh.blocks(g, 5, 3, 2)
    assert [b[k].shape for k in uh.BLOCKS] == [(5, 3), (3,), (3, 2), (2,)]
    assert np.array_equal(np.concatenate([b[k].ravel() for k in uh.BLOCKS]), g)
    W1, b1, W2, b2 = ho.unpack(g, 5, 3, 2)
    assert np.array_equal(b["dW1"], W1) and np.array_equal(b["db2"], b2)


def test_chunks_per_wave_table():
    """The in list of the forward sweep, recomputed from the kernel's two lines of arithmetic."""
    table = {16: (1, 0, 0, 0), 48: (1, 1, 1, 0), 64: (1, 1, 1, 1), 80: (2, 2, 1, 0), 192: (3, 3, 3, 3), 208: (4, 4, 4, 1),
             320: (5,) * 4, 448: (7,) * 4, 512: (8,) * 4, 576: (9,) * 4, 1040: (17, 17, 17, 14), 1024: (16,) * 4,
             1280: (20,) * 4, 2048: (32,) * 4}
    assert set(table) == set(uh.MFMA_INS)
    seen = set()
    for in_dim, want in table.items():
        assert uh.mfma_chunks_per_wave(in_dim) == want, in_dim
        assert sum(want) == in_dim // 16
        assert sum((uh.mfma_wave_chunks(in_dim, w) for w in range(4)), []) == list(range(in_dim // 16))
        seen.update(want)
    assert {0, 1, 2, 3, 4, 5, 7, 8}.issubset(seen) and max(seen) >= 9


def test_forward_table_covers_the_paths():
    dims = uh.FORWARD_DIMS
    assert len(set(dims)) == len(dims)
    assert {d[0] for d in dims} == set(uh.MFMA_INS) | set(uh.ROWS_INS)
    assert {(d[1], d[2]) for d in dims} >= {(h, c) for h in uh.HIDDENS for c in uh.CLASSES}
    for kind in (lambda i: i % 16 == 0, lambda i: i % 16 != 0):
        sub = [d for d in dims if kind(d[0])]
        assert {d[1] for d in sub} == set(uh.HIDDENS) and {d[2] for d in sub} == set(uh.CLASSES)
    assert any(d[0] % 16 and d[1] % 2 for d in dims)
    # fewer than 4 chunks, exactly 4, 5..7 and the steady state, each on both tile counts (hidden <= 16 / > 16)
    for nt_two in (False, True):
        got = set()
        for d in dims:
            if d[0] % 16 == 0 and (d[1] > 16) == nt_two:
                got.update(uh.mfma_chunks_per_wave(d[0]))
        assert got & {1, 2, 3} and got & {5, 6, 7} and got & set(range(8, 40)), (nt_two, got)
    assert all(set(uh.REGIME_DIMS) <= s for s in ({d for d, r in uh.forward_cases() if r == reg} for reg in ("loud", "saturated")))
    assert all(d in uh.GRAD_DIMS or d[1] == 16 for d in uh.REGIME_DIMS)


def test_saturated_recipe_is_saturated():
    for dims in uh.REGIME_DIMS:
        case = uh.Case(*dims, 257, "saturated")
        W1, b1, _, _ = [a.astype(np.float64) for a in ho.unpack(case.p, *dims)]
        pre = case.x.astype(np.float64) @ W1 + b1
        r = case.ref()
        assert np.abs(pre).max() > 20 and (np.abs(pre) > 9).mean() > 0.3
        assert r.probs.min() < 1e-45 and r.loss_rows.max() > 50
        assert np.array_equal(case.ref(np.float32).probs.argmax(1), r.probs.argmax(1))


# ---- the float32 oracle passes every case the GPU file runs -----------------------------------------------------------------------

@pytest.mark.parametrize("spec", uh.forward_cases(), ids=uh.case_id)
def test_float32_oracle_passes_forward_case(spec):
    case = uh.forward_case(*spec)
    uh.check_probs(case.ref(np.float32).probs, case)
    assert not case.tie_rows().any()


@pytest.mark.parametrize("spec", uh.grad_cases(), ids=uh.case_id)
def test_float32_oracle_passes_gradient_case(spec):
    case = uh.Case(*spec[0], *spec[1:])
    r32 = case.ref(np.float32)
    uh.check_gradient(r32.g, case)
    uh.check_loss_sum(r32.loss_sum, case)
    uh.check_ncorrect(float(r32.ncorrect), case)
    assert not case.tie_rows().any()
    if case.regime == "zero_feature":
        assert np.abs(case.ref().dW1).max() > 0


@pytest.mark.parametrize("dims", uh.MANY_HEADS_CASES, ids=uh.case_id)
def test_float32_oracle_passes_many_heads_case(dims):
    case, params = uh.many_heads_case(dims)
    uh.check_probs(case.ref(np.float32).probs, case)
    assert not case.tie_rows().any()
    assert len(params) == 129 and len({p.tobytes() for p in params}) == 129 and params[0] is case.p
    kinds = [(d[0] % 16 == 0, d[1] > 16) for d in uh.MANY_HEADS_CASES]
    assert (True, False) in kinds and (True, True) in kinds and sum(1 for k in kinds if not k[0]) == 2
    assert max(uh.MANY_HEADS_COUNTS) == 2 * 64 + 1 and 64 in uh.MANY_HEADS_COUNTS and 65 in uh.MANY_HEADS_COUNTS


def test_gradient_table_reaches_the_edges():
    cases = uh.grad_cases()
    assert {c[0] for c in cases if c[2] in ("ordinary", "zero_feature")} == set(uh.GRAD_DIMS)
    for d in uh.GRAD_DIMS:
        assert {c[1] for c in cases if c[0] == d and c[2] in ("ordinary", "zero_feature")} >= set(uh.GRAD_BATCHES)
        assert {c[3] for c in cases if c[0] == d} == set(uh.LABEL_KINDS)
    def last_slice(B):                       # rows_per = ceil(B / 32), splits = ceil(B / rows_per): what mkws_head_loss_grad launches
        rows_per = -(-B // 32)
        return B - (-(-B // rows_per) - 1) * rows_per
    assert [last_slice(B) for B in (33, 65, 97, 511)] == [1, 2, 1, 15]
    d, B = uh.BIG_GRAD
    rows_per = -(-B // 32)
    assert (d, B) in {(c[0], c[1]) for c in cases} and rows_per > 64 and B - 31 * rows_per == 54 and B <= uh.MAX_BATCH
    assert all(c[1] <= uh.MAX_BATCH for c in cases)


@pytest.mark.parametrize("spec", uh.INPUT_GRAD_CASES, ids=uh.case_id)
def test_float32_oracle_passes_input_grad_case(spec):
    dims, B, regime = spec
    case = uh.Case(*dims, B, regime)
    uh.assert_close(case.ref(np.float32).dX, case, "dX")
    # and a dX that forgets the last hidden unit does not
    W1 = ho.unpack(case.p, *dims)[0].astype(np.float64)
    mutant = case.ref().dpre[:, :-1] @ W1[:, :-1].T
    assert rejected(uh.assert_close, mutant, case, "dX", margin=10 * uh.margin_for(case, "dX"))
    assert sum(1 for d, b, _ in uh.INPUT_GRAD_CASES if b * d[0] > 1048576) >= 2


@pytest.mark.parametrize("setting", sorted(uh.ADAM_SETTINGS))
@pytest.mark.parametrize("first_t,steps", [(1, uh.ADAM_STEPS), (1000, 1), (100000, 1)])
def test_float32_oracle_passes_adam_case(setting, first_t, steps):
    ac = uh.AdamCase(setting, steps=steps, first_t=first_t)
    ac.assert_close(ac.trajectory(np.float32))
    moved = np.ones(len(ac.p0), bool)
    moved[ac.untouched()] = False
    assert np.all(ac.trajectory()[~moved] == ac.p0[~moved]) and np.mean(ac.trajectory()[moved] != ac.p0[moved]) > 0.99
