"""Comparators, input recipes and case tables for the few-shot head tests (plain numpy, no GPU).

The yardstick of every comparison is the ROUND-OFF UNIT of the quantity compared: the error of
oracle/head_oracle.py evaluated in float32 against its own float64 run on the same float32 inputs,
normalised per quantity (probabilities absolute; each gradient block by that block's own float64 max;
the loss sum relative to max(|loss sum|, 1); dX by its own max; Adam parameters absolute).  A kernel
passes when   error <= MARGIN[quantity] * unit * normaliser + FLOOR_ULPS * eps32 * normaliser.
No tolerance here is taken from the code under test; tests/test_head_checks_cpu.py proves that
structural mistakes (a forgotten row, a skipped K chunk, ...) land orders of magnitude outside.

tests/test_head_paths_gpu.py (device) and tests/test_head_checks_cpu.py (no GPU) import the SAME case
tables from here, so what the CPU file vets is what the GPU file runs.
"""
import numpy as np

from oracle import head_oracle as ho

EPS32 = float(np.finfo(np.float32).eps)

# kernel error / round-off unit allowed per quantity.  4 is the starting point for all of them: the kernels add
# the same float32 terms in another order than numpy/BLAS (MFMA K chunks, four-wave split, 32 row slices).
MARGIN = {"probs": 4.0, "dW1": 4.0, "db1": 4.0, "dW2": 4.0, "db2": 4.0, "loss_sum": 4.0, "dX": 4.0, "adam": 4.0}
# Measured above 4 on the MI355X, in the saturated regime only: twice the worst measured ratio (profiles/head_paths_accuracy.txt
# has every ratio and the reason: with |pre| up to 47 one float32 ulp of a pre-activation is 4e-6, only the handful of rows
# that are not one-hot carry any error at all, and the unit of a small batch is ONE draw of that error with BLAS's summation
# order -- re-ordering the float32 sum in numpy moves it by 15x either way).  The smallest mutant of
# tests/test_head_checks_cpu.py in these quantities sits at 44 000 units (probs) and stays rejected at ten times these margins.
MARGIN_SATURATED = {"probs": 32.1, "dW1": 12.2, "db1": 12.1}


def margin_for(case, quantity):
    if getattr(case, "regime", None) == "saturated" and quantity in MARGIN_SATURATED:
        return MARGIN_SATURATED[quantity]
    return MARGIN[quantity]


# a few float32 ulps of the normaliser: tiny cases (B = 1, in = 16) have a unit that is one draw of a handful of
# roundings and can come out as 0
FLOOR_ULPS = 4.0

TIE_GAP = 1e-5      # rows whose float64 top-two logit gap is below this are left out of argmax / ncorrect equality
TIE_CAP = 0.01      # at most this fraction of a case's rows may be left out (a condition on the seeds, asserted)

REGIMES = ("ordinary", "loud", "saturated", "zero_feature")
LABEL_KINDS = ("uniform", "one_class", "absent")
BLOCKS = ("dW1", "db1", "dW2", "db2")

RECORDS = []        # (case id, quantity, error / normaliser, unit, margin) of every assert_close call, for the accuracy profile


def nparams(in_dim, hid, cls):
    return in_dim * hid + hid + hid * cls + cls


def blocks(g, in_dim, hid, cls):
    """A flat gradient (or parameter vector) as {dW1, db1, dW2, db2}."""
    g = np.asarray(g)
    assert g.shape == (nparams(in_dim, hid, cls),), g.shape
    o1 = in_dim * hid
    o2 = o1 + hid
    o3 = o2 + hid * cls
    return {"dW1": g[:o1].reshape(in_dim, hid), "db1": g[o1:o2], "dW2": g[o2:o3].reshape(hid, cls), "db2": g[o3:]}


def logits(p, x, dims, dtype=np.float64):
    W1, b1, W2, b2 = [a.astype(dtype) for a in ho.unpack(np.asarray(p), *dims)]
    h = np.tanh(np.asarray(x, dtype=dtype) @ W1 + b1)
    return h @ W2 + b2, h


def loss_from_logits(p, x, y, dims, dtype=np.float64):
    """Row losses as logsumexp(z) - z_y (what Keras computes for a softmax output; finite where -log(p_y) overflows)."""
    z, _ = logits(p, x, dims, dtype)
    zmax = z.max(axis=1)
    lse = zmax + np.log(np.exp(z - zmax[:, None]).sum(axis=1))
    return lse - z[np.arange(z.shape[0]), np.asarray(y)]


def zero_columns(in_dim):
    return np.unique(np.concatenate([np.arange(0, in_dim, 5), [in_dim - 1]]))


def recipe_params(rng, dims, regime):
    """Glorot weights with non-zero biases; `saturated` scales W1 by 30 and W2 by 25."""
    in_dim, hid, cls = dims
    l1, l2 = np.sqrt(6.0 / (in_dim + hid)), np.sqrt(6.0 / (hid + cls))
    W1 = rng.uniform(-l1, l1, (in_dim, hid))
    b1 = 0.1 * rng.standard_normal(hid)
    W2 = rng.uniform(-l2, l2, (hid, cls))
    b2 = 0.1 * rng.standard_normal(cls)
    if regime == "saturated":
        W1, W2 = W1 * 30.0, W2 * 25.0
    return np.concatenate([W1.ravel(), b1, W2.ravel(), b2]).astype(np.float32)


def recipe_inputs(rng, dims, B, regime, labels):
    in_dim, _, cls = dims
    x = ((3.0 if regime == "loud" else 0.3) * rng.standard_normal((B, in_dim))).astype(np.float32)
    if regime == "zero_feature":
        x[:, zero_columns(in_dim)] = 0.0
    if labels == "uniform":
        y = rng.integers(0, cls, B)
    elif labels == "one_class":
        y = np.full(B, int(rng.integers(0, cls)))
    else:                                           # one class never appears
        y = (int(rng.integers(0, cls)) + 1 + rng.integers(0, cls - 1, B)) % cls
    return x, y.astype(np.int32)


def case_seed(dims, B, regime, labels, salt=0):
    return (dims[0] * 1000003 + dims[1] * 10007 + dims[2] * 101 + B * 7 + REGIMES.index(regime) * 3 + LABEL_KINDS.index(labels)
            + salt * 7919) % (2 ** 31)


# cases whose first seed puts a row of the float64 reference within TIE_GAP of a tie draw again with this salt
# (the near-tie cap is a condition on the seeds: tests/test_head_checks_cpu.py asserts that no case of the tables has such a row)
SALTS = {((1, 18, 5), 37, "ordinary", "uniform"): 1, ((320, 32, 8), 511, "loud", "one_class"): 1}


class Case:
    """float32 parameters p, inputs x [B, in], labels y, and the oracle's results on them in either precision."""

    def __init__(self, in_dim, hid, cls, B, regime="ordinary", labels="uniform", salt=None):
        assert regime in REGIMES and labels in LABEL_KINDS
        self.dims, self.B, self.regime, self.labels = (in_dim, hid, cls), B, regime, labels
        salt = SALTS.get((self.dims, B, regime, labels), 0) if salt is None else salt
        rng = np.random.default_rng(case_seed(self.dims, B, regime, labels, salt))
        self.p = recipe_params(rng, self.dims, regime)
        self.x, self.y = recipe_inputs(rng, self.dims, B, regime, labels)
        self.id = "%dx%dx%d-B%d-%s-%s" % (in_dim, hid, cls, B, regime, labels)
        self._ref = {}

    def ref(self, dtype=np.float64):
        """The oracle on this case: probs, z, h, dW1 | db1 | dW2 | db2, loss_sum, ncorrect, dpre, dX (dX computed on demand)."""
        key = np.dtype(dtype).name
        if key not in self._ref:
            self._ref[key] = _Ref(self, dtype)
        return self._ref[key]

    def tie_rows(self):
        """Rows whose float64 top-two logit gap is below TIE_GAP."""
        z = np.sort(self.ref().z, axis=1)
        return (z[:, -1] - z[:, -2]) < TIE_GAP


class _Ref:
    def __init__(self, case, dtype):
        d = case.dims
        self.probs, self.h = ho.forward(case.p, case.x, *d, dtype=dtype)
        with np.errstate(divide="ignore"):           # float32 -log(p) is inf once p underflows (saturated); not used as a yardstick
            _, g, self.ncorrect, self.loss_sum_via_log = ho.loss_and_grad(case.p, case.x, case.y, *d, dtype=dtype)
        self.g = g
        for k, v in blocks(g, *d).items():
            setattr(self, k, v)
        self.z, _ = logits(case.p, case.x, d, dtype)
        self.loss_rows = loss_from_logits(case.p, case.x, case.y, d, dtype)
        self.loss_sum = self.loss_rows.sum()
        self._case, self._dtype = case, dtype

    @property
    def dpre(self):
        c, dt = self._case, self._dtype
        _, _, W2, _ = [a.astype(dt) for a in ho.unpack(c.p, *c.dims)]
        dz = self.probs.copy()
        dz[np.arange(c.B), c.y] -= 1.0
        dz /= c.B
        return (dz @ W2.T) * (1.0 - self.h * self.h)

    @property
    def dX(self):
        c, dt = self._case, self._dtype
        W1 = ho.unpack(c.p, *c.dims)[0].astype(dt)
        return self.dpre @ W1.T


def normaliser(ref64_value, quantity):
    if quantity in ("probs", "adam"):
        return 1.0
    if quantity == "loss_sum":
        return max(abs(float(ref64_value)), 1.0)
    return float(np.abs(ref64_value).max())


def deviation(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float(d.max()) if d.size else 0.0


def roundoff_unit(case, quantity):
    """Error of the float32 oracle against the float64 oracle on `case`, divided by the quantity's normaliser."""
    r64 = getattr(case.ref(np.float64), quantity)
    n = normaliser(r64, quantity)
    return deviation(getattr(case.ref(np.float32), quantity), r64) / n if n > 0 else 0.0


def compare(got, want64, unit, quantity, label, margin=None):
    """The comparison behind assert_close, with the unit supplied (Adam trajectories bring their own)."""
    margin = MARGIN[quantity] if margin is None else margin
    n = normaliser(want64, quantity)
    got = np.asarray(got)
    assert got.shape == np.shape(want64), (label, quantity, got.shape, np.shape(want64))
    err = deviation(got, want64)
    rel = err / n if n > 0 else err
    RECORDS.append((label, quantity, rel, unit, margin))
    tol = (margin * unit + FLOOR_ULPS * EPS32) * n
    ok = bool(np.all(np.isfinite(got))) and err <= tol          # nan / inf never pass
    assert ok, "%s %s: error %.3e (%.3e of the normaliser %.3e) > %g x unit %.3e + %g ulp floor" % (
        label, quantity, err, rel, n, margin, unit, FLOOR_ULPS)
    return rel / unit if unit > 0 else (0.0 if rel == 0 else float("inf"))


def assert_close(got, case, quantity, margin=None):
    """got (a kernel result, or a mutated oracle result) against the float64 oracle's `quantity` on `case`."""
    margin = margin_for(case, quantity) if margin is None else margin
    return compare(got, getattr(case.ref(np.float64), quantity), roundoff_unit(case, quantity), quantity, case.id, margin)


def assert_tie_cap(case):
    """At most TIE_CAP of the rows may sit on a near-tie; returns the mask of the rows left out."""
    tie = case.tie_rows()
    assert tie.sum() <= TIE_CAP * case.B, "%s: %d of %d rows within %g of a tie: pick another seed" % (case.id, tie.sum(), case.B, TIE_GAP)
    return tie


def check_probs(probs, case):
    """Forward checks: the unit, rows summing to 1, argmax, and what the saturated regime may do to small values."""
    probs = np.asarray(probs)
    cls = case.dims[2]
    ref = case.ref(np.float64)
    assert probs.dtype == np.float32 and np.all(np.isfinite(probs)) and probs.min() >= 0.0, case.id
    assert_close(probs, case, "probs")
    # p_k = fl(e_k * inv), inv = fl(1 / fl(sum e)): the float32 sum of cls terms is off by at most (cls - 1) u relative,
    # inv and each product by u more  (u = eps32 / 2)  ->  |sum p - 1| <= (cls + 1) u; one more u for slack
    rowsum = probs.astype(np.float64).sum(axis=1)
    assert np.abs(rowsum - 1.0).max() <= (cls + 2) * EPS32 / 2, (case.id, np.abs(rowsum - 1.0).max())
    keep = ~assert_tie_cap(case)
    assert np.array_equal(probs.argmax(1)[keep], ref.probs.argmax(1)[keep]), case.id
    # exact zeros are fine where float32 cannot hold the value: below its smallest denormal 2^-149 = 1.4e-45 a result is 0 or 2^-149,
    # and an exp that is good to one unit in the last place may give either (the device's expf gives 0 up to 1.39e-45, measured);
    # from two denormal steps on, a zero would be wrong by two units of the format
    assert not np.any((probs == 0.0) & (ref.probs >= 2.0 ** -148)), (case.id, ref.probs[probs == 0.0].max())


def check_ncorrect(ncorrect, case):
    """Exact, up to the near-tie rows."""
    n_tie = int(assert_tie_cap(case).sum())
    assert float(ncorrect) == int(ncorrect), (case.id, ncorrect)
    assert abs(int(ncorrect) - case.ref(np.float64).ncorrect) <= n_tie, (case.id, ncorrect, case.ref(np.float64).ncorrect, n_tie)


def check_gradient(g, case):
    """Every block against its own unit; zeroed input features give exactly-zero rows of dW1."""
    got = blocks(np.asarray(g), *case.dims)
    failed = []
    for name in BLOCKS:                                  # all four are measured before any of them fails the case
        try:
            assert_close(got[name], case, name)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    if case.regime == "zero_feature":
        assert np.all(got["dW1"][zero_columns(case.dims[0])] == 0.0), case.id


def check_loss_sum(loss_sum, case):
    assert np.isfinite(loss_sum), (case.id, loss_sum)
    assert_close(np.float64(loss_sum), case, "loss_sum")


# ---- the MFMA forward kernel's K split (mkws_head.hip: kper = ceil(KC / 4), wave w walks [w kper, (w + 1) kper) ∩ [0, KC)) ----

def mfma_chunks_per_wave(in_dim):
    assert in_dim % 16 == 0
    kc = in_dim // 16
    kper = (kc + 3) // 4
    return tuple(max(0, min(kper, kc - w * kper)) for w in range(4))


def mfma_wave_chunks(in_dim, wave):
    """The 16-feature chunk indices wave `wave` accumulates, ascending."""
    kper = (in_dim // 16 + 3) // 4
    return list(range(wave * kper, wave * kper + mfma_chunks_per_wave(in_dim)[wave]))


# ---- case tables -------------------------------------------------------------------------------------------------------------

MFMA_INS = (16, 48, 64, 80, 192, 208, 320, 448, 512, 576, 1040, 1024, 1280, 2048)
ROWS_INS = (1, 7, 63, 65, 100, 1000, 1030)
HIDDENS = (1, 2, 15, 16, 17, 18, 31, 32)
CLASSES = (2, 3, 5, 8)
FORWARD_BATCH = 37
FORWARD_PREFIXES = (1, 15, 16, 17)

# every (hidden, classes) pair once, the in values dealt round (MFMA and rows-kernel widths alternating) ...
FORWARD_DIMS = [
    (16, 1, 2), (1, 1, 3), (48, 1, 5), (7, 1, 8),
    (64, 2, 2), (63, 2, 3), (80, 2, 5), (65, 2, 8),
    (192, 15, 2), (100, 15, 3), (208, 15, 5), (1000, 15, 8),
    (320, 16, 2), (1030, 16, 3), (448, 16, 5), (512, 16, 8),
    (576, 17, 2), (1040, 17, 3), (1024, 17, 5), (1280, 17, 8),
    (2048, 18, 2), (16, 18, 3), (1, 18, 5), (48, 18, 8),
    (7, 31, 2), (64, 31, 3), (63, 31, 5), (80, 31, 8),
    (65, 32, 2), (192, 32, 3), (100, 32, 5), (208, 32, 8),
    # ... plus the widths the product creates and both sides of the NT = 1 / 2 switch on the rows kernels
    (1024, 18, 3), (1280, 18, 3), (2048, 18, 3), (192, 18, 3), (100, 17, 5), (63, 16, 3), (1030, 17, 2), (320, 32, 8),
]

GRAD_DIMS = [(1024, 18, 3), (1280, 18, 3), (2048, 18, 3), (192, 18, 3), (100, 17, 5), (320, 32, 8), (63, 16, 3), (16, 1, 2)]
GRAD_BATCHES = (1, 2, 31, 32, 33, 63, 65, 97, 200, 511)
BIG_GRAD = ((1024, 18, 3), 2100)          # second 64-row chunk of a row slice (rows_per = 66) and a 54-row last slice
REGIME_DIMS = [(1024, 18, 3), (192, 16, 3), (100, 17, 5), (320, 32, 8)]
MAX_BATCH = 2100


def forward_cases():
    """(dims, regime) of sections a and d: every case is FORWARD_BATCH rows, its prefixes are the smaller batches."""
    return [(d, "ordinary") for d in FORWARD_DIMS] + [(d, r) for r in ("loud", "saturated") for d in REGIME_DIMS]


def forward_case(dims, regime):
    return Case(*dims, FORWARD_BATCH, regime, "uniform")


def grad_cases():
    """(dims, B, regime, labels) of sections c and d.  Ordinary cases alternate with zero_feature ones; the label sets rotate."""
    out = []
    for di, d in enumerate(GRAD_DIMS):
        for bi, B in enumerate(GRAD_BATCHES):
            out.append((d, B, "zero_feature" if bi % 2 else "ordinary", LABEL_KINDS[(di + bi) % 3]))
    out.append((BIG_GRAD[0], BIG_GRAD[1], "zero_feature", "uniform"))
    for r in ("loud", "saturated"):
        for di, d in enumerate(REGIME_DIMS):
            for bi, B in enumerate(GRAD_BATCHES):
                out.append((d, B, r, LABEL_KINDS[(di + bi + 1) % 3]))
    return out


def case_id(spec):
    return "-".join("x".join(map(str, s)) if isinstance(s, tuple) else str(s) for s in spec)


# (dims, B, regime): the grid-stride loop (more than 1 048 576 elements), in % 256 != 0 with odd hidden, saturated once
INPUT_GRAD_CASES = [((1024, 18, 3), 1025, "ordinary"), ((2048, 18, 3), 513, "ordinary"), ((100, 17, 5), 37, "ordinary"),
                    ((1024, 18, 3), 200, "saturated")]

# (dims, B of the sweep) of section b: one MFMA case per NT, two rows-kernel cases (odd and even hidden)
MANY_HEADS_CASES = [(192, 16, 3), (1024, 18, 3), (100, 17, 5), (1030, 18, 2)]
MANY_HEADS_COUNTS = (1, 64, 65, 129)
MANY_HEADS_BATCHES = (1, 15, 16, 17, 37)


def many_heads_case(dims):
    """The shared inputs (a Case whose parameters are the first head's) and the parameters of all the heads."""
    case = Case(*dims, max(MANY_HEADS_BATCHES), salt=100)
    rng = np.random.default_rng(dims[0] + 31 * dims[1])
    return case, [case.p] + [recipe_params(rng, dims, "ordinary") for _ in range(max(MANY_HEADS_COUNTS) - 1)]


# ---- Adam ----------------------------------------------------------------------------------------------------------------------

ADAM_DIMS, ADAM_BATCH, ADAM_STEPS, ADAM_LR = (1024, 18, 3), 200, 30, 1e-3
ADAM_SETTINGS = {
    "default": dict(beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0),
    "fast_betas": dict(beta1=0.5, beta2=0.9, eps=1e-3, grad_scale=0.5),
}


class AdamCase:
    """Starting parameters and `steps` fresh zero_feature batches (the same features are zero in every batch, so
    those rows of W1 never see a gradient)."""

    def __init__(self, setting, steps=ADAM_STEPS, first_t=1):
        self.setting, self.opts, self.first_t = setting, ADAM_SETTINGS[setting], first_t
        rng = np.random.default_rng(4242 + sorted(ADAM_SETTINGS).index(setting) + 17 * first_t)
        self.dims = ADAM_DIMS
        self.p0 = recipe_params(rng, self.dims, "ordinary")
        self.batches = [recipe_inputs(rng, self.dims, ADAM_BATCH, "zero_feature", "uniform") for _ in range(steps)]
        self.id = "adam-%s-t%d-%dsteps" % (setting, first_t, steps)
        self._traj = {}

    def untouched(self):
        """Indices of the parameters whose gradient is exactly zero in every step."""
        hid = self.dims[1]
        return (zero_columns(self.dims[0])[:, None] * hid + np.arange(hid)[None, :]).ravel()

    def trajectory(self, dtype=np.float64, adam_cls=ho.KerasAdam):
        """Parameters after the last step of oracle gradients fed to `adam_cls`, everything held in `dtype`."""
        key = (np.dtype(dtype).name, adam_cls)
        if key not in self._traj:
            o = self.opts
            opt = adam_cls(len(self.p0), lr=ADAM_LR, beta1=o["beta1"], beta2=o["beta2"], eps=o["eps"], dtype=dtype)
            opt.t = self.first_t - 1
            p = self.p0.astype(dtype)
            for x, y in self.batches:
                g = ho.loss_and_grad(p, x, y, *self.dims, dtype=dtype)[1] * dtype(o["grad_scale"])
                p = opt.step(p, g).astype(dtype)
            self._traj[key] = p
        return self._traj[key]

    def unit(self):
        return deviation(self.trajectory(np.float32), self.trajectory(np.float64))

    def assert_close(self, got, margin=None):
        return compare(got, self.trajectory(np.float64), self.unit(), "adam", self.id, margin)


def write_records(path, note=""):
    """The accuracy profile: error / normaliser, unit and their ratio of every comparison made so far."""
    with open(path, "w") as f:
        f.write("# %s\n" % note)
        f.write("# case quantity error_over_normaliser unit ratio ratio_after_floor margin\n")
        for label, q, rel, unit, margin in RECORDS:
            ratio = rel / unit if unit > 0 else (0.0 if rel == 0 else float("inf"))
            after = max(0.0, rel - FLOOR_ULPS * EPS32) / unit if unit > 0 else (0.0 if rel <= FLOOR_ULPS * EPS32 else float("inf"))
            f.write("%s %s %.3e %.3e %.2f %.2f %g\n" % (label, q, rel, unit, ratio, after, margin))
