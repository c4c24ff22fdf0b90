"""-m gpu: head.HeadGroup (mkws_head_group_*: K keyword heads stepped by one set of launches) against the single-head entry points.

Every comparison is EXACT: np.array_equal on state_view() (params | grads + statistics | Adam m | Adam v) and == on the returned
statistics, against separately created Heads that hold the same parameters and see the same rows through Head.loss_grad +
Head.adam_step.  tests/test_head_paths_gpu.py holds the single-head path to the float64 oracle; bit-equality carries that over, and
one test below repeats the oracle check on the group path with cases of the vetted tables (tests/test_head_checks_cpu.py)."""
import numpy as np
import pytest

from tests import util_head as uh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DIMS = [(1024, 18, 3), (100, 17, 5), (320, 32, 8), (16, 1, 2)]       # all in uh.GRAD_DIMS
BATCHES = (1, 2, 31, 33, 65, 97)                                    # all in uh.GRAD_BATCHES
GROUP_SIZES = (1, 2, 5)
CHUNK = 64                                                          # kGroupHeadsPerLaunch (mkws_head.hip)
MAX_BATCH = 128
LR = 1e-3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def head_case(dims, B, h):
    """Head h's own parameters and data: util_head's recipe under a salt of its own."""
    return uh.Case(*dims, B, salt=1000 + h)


def make_heads(dims, n, dev, max_batch=MAX_BATCH):
    from multilingual_kws_amd.head import Head
    return [Head(*dims, max_batch=max_batch, seed=h, device=dev) for h in range(n)]


@pytest.fixture(scope="module")
def pools(dev):
    """Per dimension triple: max(GROUP_SIZES) heads for the group path, as many for the single-head path, one HeadGroup per size."""
    from multilingual_kws_amd.head import HeadGroup
    cache = {}

    def get(dims):
        if dims not in cache:
            n = max(GROUP_SIZES)
            grouped, single = make_heads(dims, n, dev), make_heads(dims, n, dev)
            cache[dims] = (grouped, single, {k: HeadGroup(grouped[:k]) for k in GROUP_SIZES})
        return cache[dims]

    yield get
    torch.cuda.synchronize()
    for grouped, single, groups in cache.values():
        for g in groups.values():
            g.close()
        for hd in grouped + single:
            hd.close()


def single_round(hd, x, y, **adam):
    """One single-head step -> (statistics, state after it)."""
    stats = hd.loss_grad(x, y).tolist()
    hd.adam_step(lr=LR, **adam)
    return stats, hd.state_view().cpu().numpy().copy()


def stacked(cases, dev):
    return (torch.from_numpy(np.stack([c.x for c in cases])).to(dev), torch.from_numpy(np.stack([c.y for c in cases])).to(dev))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("dims", DIMS, ids=uh.case_id)
def test_one_round_equals_single_heads(dev, pools, dims, B):
    grouped, single, groups = pools(dims)
    cases = [head_case(dims, B, h) for h in range(len(single))]
    want = []
    for hd, c in zip(single, cases):                    # the reference, once for all group sizes
        hd.set_params(c.p)
        want.append(single_round(hd, torch.from_numpy(c.x).to(dev), torch.from_numpy(c.y).to(dev)))
    for K in GROUP_SIZES:
        for hd, c in zip(grouped[:K], cases):
            hd.set_params(c.p)
        emb, labels = stacked(cases[:K], dev)
        stats = groups[K].loss_grad(emb, labels, rows=B)
        assert stats.shape == (K, 2)
        stats = stats.tolist()
        groups[K].adam_step(lr=LR)
        for h in range(K):
            assert stats[h] == want[h][0], (dims, B, K, h)
            assert grouped[h].step_t == 1
            assert np.array_equal(grouped[h].state_view().cpu().numpy(), want[h][1]), (dims, B, K, h)


def test_group_larger_than_one_launch(dev):
    """K = CHUNK + 1 heads: the second launch of every stage takes its own slots, rows, labels and statistics."""
    from multilingual_kws_amd.head import HeadGroup
    dims, B, K = (16, 1, 2), 5, CHUNK + 1
    cases = [head_case(dims, B, h) for h in range(K)]
    grouped, single = make_heads(dims, K, dev, 8), make_heads(dims, K, dev, 8)
    group = HeadGroup(grouped)
    try:
        assert len(group) == K and group.L.mkws_head_group_size(group.h) == K
        for g, s, c in zip(grouped, single, cases):
            g.set_params(c.p)
            s.set_params(c.p)
        emb, labels = stacked(cases, dev)
        stats = group.loss_grad(emb, labels).tolist()           # rows=None: all of them
        group.adam_step(lr=LR, beta1=0.5, beta2=0.9, eps=1e-3, grad_scale=0.5)
        for h in range(K):
            st, state = single_round(single[h], torch.from_numpy(cases[h].x).to(dev), torch.from_numpy(cases[h].y).to(dev),
                                     beta1=0.5, beta2=0.9, eps=1e-3, grad_scale=0.5)
            assert stats[h] == st, h
            assert np.array_equal(grouped[h].state_view().cpu().numpy(), state), h
        assert len({tuple(s) for s in stats}) > 1               # the heads really differ
    finally:
        group.close()
        for hd in grouped + single:
            hd.close()


@pytest.mark.parametrize("dims,B", [((1024, 18, 3), 33), ((100, 17, 5), 2)], ids=["1024x18x3-B33", "100x17x5-B2"])
def test_strided_slabs_read_only_their_rows(dev, pools, dims, B):
    """emb [K, 3 B, in] / labels [K, 3 B] with offset = B: the rows around the selected ones are NaN / -1 and must not be looked at."""
    K = 2
    grouped, single, groups = pools(dims)
    cases = [head_case(dims, B, 10 + h) for h in range(K)]
    emb = torch.full((K, 3 * B, dims[0]), float("nan"), dtype=torch.float32, device=dev)
    labels = torch.full((K, 3 * B), -1, dtype=torch.int32, device=dev)
    x, y = stacked(cases, dev)
    emb[:, B:2 * B], labels[:, B:2 * B] = x, y
    for h in range(K):
        grouped[h].set_params(cases[h].p)
        single[h].set_params(cases[h].p)
    stats = groups[K].loss_grad(emb, labels, rows=B, offset=B).tolist()
    groups[K].adam_step(lr=LR)
    for h in range(K):
        st, state = single_round(single[h], x[h], y[h])
        assert np.all(np.isfinite(state)) and stats[h] == st, (h, stats[h], st)
        assert np.array_equal(grouped[h].state_view().cpu().numpy(), state), h


def test_five_consecutive_rounds(dev, pools):
    dims, B, K, rounds = (1024, 18, 3), 33, 3, 5
    grouped, single, _ = pools(dims)
    from multilingual_kws_amd.head import HeadGroup
    group = HeadGroup(grouped[1:1 + K])                 # a group need not start at the pool's first head
    members, refs = grouped[1:1 + K], single[:K]
    data = [[head_case(dims, B, 100 + 10 * r + h) for h in range(K)] for r in range(rounds)]
    for h in range(K):
        members[h].set_params(data[0][h].p)
        refs[h].set_params(data[0][h].p)
    try:
        for r in range(rounds):
            emb, labels = stacked(data[r], dev)
            stats = group.loss_grad(emb, labels, rows=B).tolist()
            group.adam_step(lr=LR)
            for h in range(K):
                st, state = single_round(refs[h], emb[h], labels[h])
                assert stats[h] == st, (r, h)
                assert members[h].step_t == refs[h].step_t == r + 1
                assert np.array_equal(members[h].state_view().cpu().numpy(), state), (r, h)
    finally:
        group.close()


def test_group_against_the_float64_oracle(dev, pools):
    """The three (1024,18,3) x B = 65 cases of util_head.grad_cases() (ordinary, loud, saturated), one per head of a group of three."""
    dims, B = (1024, 18, 3), 65
    specs = [s for s in uh.grad_cases() if s[0] == dims and s[1] == B]
    assert len(specs) == 3
    cases = [uh.Case(*s[0], *s[1:]) for s in specs]
    grouped, _, groups = pools(dims)
    from multilingual_kws_amd.head import HeadGroup
    group = HeadGroup(grouped[:3])
    try:
        for hd, c in zip(grouped, cases):
            hd.set_params(c.p)
        emb, labels = stacked(cases, dev)
        stats = group.loss_grad(emb, labels, rows=B).cpu().numpy().copy()
        for h, c in enumerate(cases):
            g = grouped[h].grad_view(with_stats=True).cpu().numpy()
            assert np.array_equal(g[-2:], stats[h])
            uh.check_loss_sum(stats[h][0], c)
            uh.check_ncorrect(stats[h][1], c)
            uh.check_gradient(g[:-2], c)
    finally:
        group.close()


def test_argument_checks(dev):
    from multilingual_kws_amd._lib import MkwsError
    from multilingual_kws_amd.head import Head, HeadGroup
    a, b = Head(64, 5, 2, max_batch=8, seed=0, device=dev), Head(64, 5, 2, max_batch=16, seed=1, device=dev)
    with pytest.raises(MkwsError):
        HeadGroup([a, b, a])                             # a duplicate head
    for other in ((64, 4, 2), (64, 5, 3), (80, 5, 2)):
        c = Head(*other, max_batch=8, seed=2, device=dev)
        with pytest.raises(MkwsError):
            HeadGroup([a, c])                            # mismatched dimensions
        c.close()
    group = HeadGroup([a, b])
    p0 = [a.get_params(), b.get_params()]
    emb = torch.zeros((2, 12, 64), dtype=torch.float32, device=dev)
    labels = torch.zeros((2, 12), dtype=torch.int32, device=dev)
    with pytest.raises(MkwsError):
        group.loss_grad(emb, labels, rows=9)             # above a's max_batch = 8 (b would take 16)
    with pytest.raises(ValueError):
        group.loss_grad(emb, labels, rows=8, offset=5)   # rows + offset > R
    with pytest.raises(ValueError):
        group.loss_grad(emb, labels, rows=0)
    with pytest.raises(ValueError):
        group.loss_grad(emb[:1], labels[:1], rows=4)     # one slab for two heads
    with pytest.raises(ValueError):
        group.loss_grad(emb, labels.long(), rows=4)
    with pytest.raises(ValueError):
        group.loss_grad(emb[:, :, :32], labels, rows=4)
    group.loss_grad(emb, labels, rows=8, offset=4)       # the largest that fits
    a.step_t = 3
    with pytest.raises(ValueError):
        group.adam_step(lr=LR)                           # heads with unequal step_t
    a.step_t = 0
    torch.cuda.synchronize()
    assert np.array_equal(a.get_params(), p0[0]) and np.array_equal(b.get_params(), p0[1])       # nothing refused touched a parameter
    group.close()
    a.close()
    b.close()


def test_group_lifetime(dev):
    from multilingual_kws_amd._lib import MkwsError
    from multilingual_kws_amd.head import Head, HeadGroup
    with pytest.raises(MkwsError):
        HeadGroup([])
    c = head_case((16, 1, 2), 5, 0)
    hd, ref = Head(16, 1, 2, max_batch=8, params=c.p, device=dev), Head(16, 1, 2, max_batch=8, params=c.p, device=dev)
    x, y = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.y).to(dev)
    group = HeadGroup([hd])
    group.loss_grad(x[None], y[None])
    group.adam_step(lr=LR)
    group.close()
    group.close()                                        # closing twice is harmless
    single_round(ref, x, y)
    st, state = single_round(hd, x, y)                   # the head outlives its group: an ordinary second step
    want_st, want = single_round(ref, x, y)
    assert hd.step_t == ref.step_t == 2
    assert st == want_st and np.array_equal(state, want)
    assert hd.forward(x).shape == (5, 2)
    hd.close()
    ref.close()
