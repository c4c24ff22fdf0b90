"""The fixed summation order of mbconv_mid_kernel's squeeze-excite tail, restated in float32 numpy and held to float64 (no GPU):
channel mean = strip sums (SEG outputs, ascending) -> slots of a channel in ascending order -> * 1 / HoWo;  reduce FC = lane l multiplies
channels l, l + 64, .. in ascending order, the 64 lane sums meet in wave_sum64_'s tree (lane pairs, quads, halves, rows of 16 by DPP, then
(r0 + r1) + (r2 + r3)).  The bound is the textbook one for a sum whose longest chain has k roundings: k u / (1 - k u) * sum |terms|,
u = 2^-24 -- nothing measured on the kernel enters it."""
import numpy as np
import pytest

U = 2.0 ** -24
F = np.float32


def _gamma(k):
    return k * U / (1 - k * U)


def _mean_f32(y, howo):
    """y [slots, SEG, C]: the outputs of every strip item, in slot order."""
    strip = np.zeros_like(y[:, 0])
    for o in range(y.shape[1]):
        strip = strip + y[:, o]
    t = strip[0]
    for sl in range(1, y.shape[0]):
        t = t + strip[sl]
    return t * F(1.0 / howo)


def _wave_sum64(v):
    lane = np.arange(64)
    for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        v = v + v[perm]
    for row in range(4):
        assert (v[16 * row:16 * row + 16].view(np.uint32) == v[16 * row].view(np.uint32)).all()      # every lane of a row holds the same bits
    return (v[0] + v[16]) + (v[32] + v[48])


def _reduce_f32(mean, wr):
    c = mean.shape[0]
    v = np.zeros(64, F)
    for i in range((c + 63) // 64):
        ch = np.arange(64) + 64 * i
        ok = ch < c
        v = v + np.where(ok, mean[np.minimum(ch, c - 1)] * wr[np.minimum(ch, c - 1)], F(0))
    return _wave_sum64(v)


@pytest.mark.parametrize("slots,seg,howo,cexp,se", [(26, 5, 130, 144, 6), (7, 5, 35, 144, 6), (4, 3, 12, 240, 10)])     # 2b, 3a, 4a
def test_fixed_order_against_float64(slots, seg, howo, cexp, se):
    rng = np.random.default_rng(slots)
    for _ in range(4):
        y = rng.standard_normal((slots, seg, cexp)).astype(F) * F(3)
        wr = rng.standard_normal((cexp, se)).astype(F)
        mean = _mean_f32(y, howo)
        assert mean.dtype == F
        y64 = y.astype(np.float64)
        mean64 = y64.sum((0, 1)) / howo
        k_mean = (seg - 1) + (slots - 1) + 2                      # strip adds, slot adds, the rounded constant 1 / HoWo and the product
        assert (np.abs(mean - mean64) <= _gamma(k_mean) * np.abs(y64).sum((0, 1)) / howo).all()
        k_fc = 1 + ((cexp + 63) // 64 - 1) + 6                    # product, a lane's adds, six tree levels
        for n in range(se):
            got = _reduce_f32(mean, wr[:, n])
            terms = mean.astype(np.float64) * wr[:, n].astype(np.float64)
            assert abs(float(got) - terms.sum()) <= _gamma(k_fc) * np.abs(terms).sum(), n
