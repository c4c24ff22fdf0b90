"""The one bank rule of multilingual_kws_amd/problems.py on the device: a read-only numpy bank, a writable one and the same bank as a CUDA
tensor give bit-identical fits in logreg.py, svc.py and kmeans.py, the device views are the host views, and a 3-D tensor is refused."""
import numpy as np
import pytest

from multilingual_kws_amd import kmeans, logreg, svc

pytestmark = pytest.mark.gpu


def test_three_routes_of_one_bank_through_the_three_fits():
    import torch
    rng = np.random.default_rng(20)
    bank = rng.normal(size=(24, 16)).astype(np.float32)
    frozen = bank.copy()
    frozen.flags.writeable = False
    rows = np.concatenate([rng.permutation(24)[:8] for _ in range(3)])
    labels = np.concatenate([rng.permutation(np.arange(8) % 3) for _ in range(3)])
    offsets = [0, 8, 16, 24]
    fits = {"logreg": lambda x: logreg.fit_on_device(x, rows, labels, offsets, 3),
            "svc": lambda x: svc.fit_on_device(x, rows, labels, offsets, 3),
            "kmeans": lambda x: kmeans.kmeans_fit_on_device(x, offsets, 2, 123)}
    for name, fit in fits.items():
        routes = [fit(frozen), fit(bank), fit(torch.from_numpy(bank).cuda())]
        assert (routes[0].info[:, 0] == 0).all(), name
        for other in routes[1:]:
            for field, a, b in zip(routes[0]._fields, routes[0], other):
                if field.startswith("d_"):
                    a, b = a.cpu().numpy(), b.cpu().numpy()
                assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()), (name, field)
        for r in routes:
            for field in r._fields:
                if field.startswith("d_"):
                    host, dev = getattr(r, field[2:]), getattr(r, field)
                    assert dev.is_cuda and tuple(dev.shape) == host.shape and dev.cpu().numpy().tobytes() == host.tobytes(), (name, field)
        with pytest.raises(ValueError):
            fit(torch.zeros((2, 12, 16), dtype=torch.float32, device="cuda"))
    assert np.array_equal(frozen, bank) and not frozen.flags.writeable
