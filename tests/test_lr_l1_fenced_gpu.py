"""mkws_lr_l1_fit called straight through the library with every pointer argument in a fenced buffer of its own (tests/util_fenced.py, the
protocol of tests/test_dataperf_fenced_gpu.py): inputs filled and apart from the outputs, outputs holding the canary NaN, the workspace
exactly as large as mkws_lr_l1_work_floats asks (no float at all: its two fences touch, and the address passed is the rear one's).

After the call: it returned 0, every fence is intact, every input is unchanged, every output element of a fitted problem is written and
has the bits the Python wrapper returns, no element of a status-2 problem beyond its info is written, and the same call again writes the
same bits.  In every bank each row that no fitted problem's list names is the canary NaN."""
import numpy as np
import pytest

import util_fenced as uf
from util_fenced import Out, protocol

pytestmark = pytest.mark.gpu

CASES = ["ragged_50_20_64", "ragged_50_20_64+label", "ragged_50_20_64+row", "n10_k2_dim1024", "n7_k3_dim37", "absent_class", "c_0p01_1_100"]
MAX_ITER, VTOL = 4000, 1e-3


def written(status, n_classes, dim):
    """status 0: coef[p], intercept[p], stats[p] and info[p] of all K classes; status 2: info[p] alone (include/mkws.h)."""
    ok = np.asarray(status) == 0
    P, K = len(ok), int(n_classes)
    wide = lambda shape: np.broadcast_to(ok.reshape((P,) + (1,) * (len(shape) - 1)), shape).copy()
    return dict(coef=wide((P, K, dim)), intercept=wide((P, K)), stats=wide((P, K, 2)), info=np.ones((P, K, 4), bool))


@pytest.mark.parametrize("name", CASES)
def test_lr_l1_fit(name):
    pytest.importorskip("torch")
    from multilingual_kws_amd import _lib, lr_l1
    c = uf.solver_case("logreg", name)
    n_bank, dim = c["x"].shape
    P, K, status = len(c["offsets"]) - 1, int(c["n_classes"]), c["status"]
    x = uf.poisoned_bank(c["x"], uf.named_rows(n_bank, (c["rows"], c["offsets"], status)))
    fit = lr_l1.fit_on_device(x, c["rows"], c["labels"], c["offsets"], K, C=c["C"], max_iter=MAX_ITER, vtol=VTOL)
    assert (fit.info[:, :, 0] == status[:, None]).all(), (name, fit.info)
    L, st = _lib.lib(), _lib.current_stream_ptr()
    n_work = int(L.mkws_lr_l1_work_floats(dim, P, K))
    assert n_work == 0
    w = written(status, K, dim)
    inputs = dict(x=x, rows=c["rows"], labels=c["labels"], offsets=c["offsets"], C=c["C"])
    outputs = {k: Out(getattr(fit, k), w[k]) for k in ("coef", "intercept", "info", "stats")}
    call = lambda p: L.mkws_lr_l1_fit(p["x"], n_bank, dim, p["rows"], p["labels"], p["offsets"], P, K, p["C"], MAX_ITER, VTOL, p["coef"], p["intercept"],
                                      p["info"], p["stats"], p["work"], n_work, st)
    got = protocol(call, inputs, outputs, work_floats=n_work)
    for q in np.nonzero(status == 2)[0]:
        assert got["info"][q].tolist() == [[2, 0, 0, 0]] * K
    assert (got["info"][status == 0][:, :, 0] == 0).all()
