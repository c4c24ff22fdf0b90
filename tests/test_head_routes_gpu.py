"""mkws_head_group_forward_routes / HeadGroup.forward_routes: route r = (slot, head) is that head of the group's table on the rows of that
slot, written to the route's own output rows.  Every valid route is held bit for bit to Head.forward of its head on its slot's rows and,
within the head tolerance of tests/util_head.py, to the float64 oracle; disabled and invalid routes to what include/mkws.h says of them."""
import functools

import numpy as np
import pytest

from multilingual_kws_amd import _lib
from tests import util_head as uh

pytestmark = pytest.mark.gpu
SLOTS, HEADS, CLASSES = 5, 6, 3
# (slot, head): head 2 on three slots; three heads on slot 2; the LAST slot twice (the row clamp at B - 1); a disabled route (its head index
# is rubbish and must not be looked at); a slot >= n_slots; a head index of -1; a head index equal to the group size
ROUTES = [(0, 2), (1, 2), (3, 2), (2, 0), (2, 1), (2, 5), (4, 3), (-1, 99), (5, 1), (1, -1), (0, 6), (4, 4)]
VALID = [r for r, (s, h) in enumerate(ROUTES) if 0 <= s < SLOTS and 0 <= h < HEADS]
INVALID = [r for r, (s, h) in enumerate(ROUTES) if s >= SLOTS or (s >= 0 and not 0 <= h < HEADS)]
DISABLED = [r for r, (s, _) in enumerate(ROUTES) if s < 0]
CANARY, PAD = -7.5, 2                                                       # PAD canary routes in front of and behind d_probs


@functools.lru_cache(maxsize=None)
def _cases(in_dim, hid, rows):
    """One util_head.Case per head over the SAME embedding rows [SLOTS * rows, in] (computed once per shape, shared, not modified)."""
    base = uh.Case(in_dim, hid, CLASSES, SLOTS * rows, salt=100)
    cases = []
    for k in range(HEADS):
        c = uh.Case(in_dim, hid, CLASSES, SLOTS * rows, salt=101 + k)
        c.x = base.x
        cases.append(c)
    return cases


def _setup(in_dim, hid, rows):
    import torch
    from multilingual_kws_amd.head import Head, HeadGroup
    cases = _cases(in_dim, hid, rows)
    B = SLOTS * rows
    heads = [Head(in_dim, hid, CLASSES, max_batch=B, params=c.p) for c in cases]
    group = HeadGroup(heads)
    emb = torch.from_numpy(cases[0].x).cuda()
    d_slot = torch.tensor([s for s, _ in ROUTES], dtype=torch.int32, device="cuda")
    d_head = torch.tensor([h for _, h in ROUTES], dtype=torch.int32, device="cuda")
    return cases, heads, group, emb, d_slot, d_head


@pytest.mark.parametrize("rows", [1, 3, 16, 17])
@pytest.mark.parametrize("hid", [16, 18, 32])
@pytest.mark.parametrize("in_dim", [32, 64, 1024])
def test_every_route_equals_its_heads_forward_on_its_slots_rows(in_dim, hid, rows):
    import torch
    cases, heads, group, emb, d_slot, d_head = _setup(in_dim, hid, rows)
    R = len(ROUTES)
    buf = torch.full((R + 2 * PAD, rows, CLASSES), CANARY, dtype=torch.float32, device="cuda")
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")             # every call that launches sets it
    probs, invalid = group.forward_routes(emb, d_slot, d_head, rows, SLOTS, out=buf[PAD:PAD + R], invalid=bad)
    assert probs.data_ptr() == buf[PAD].data_ptr() and invalid.data_ptr() == bad.data_ptr()
    assert int(bad.cpu()[0]) == len(INVALID) == 3
    assert len(VALID) == 8 and DISABLED == [7]
    host = probs.cpu().numpy()
    for r in VALID:
        s, h = ROUTES[r]
        want = heads[h].forward(emb[s * rows:(s + 1) * rows])
        assert torch.equal(probs[r], want), (r, s, h)
        ref = cases[h].ref(np.float64).probs[s * rows:(s + 1) * rows]
        uh.compare(host[r], ref, uh.roundoff_unit(cases[h], "probs"), "probs", "route %d of %s" % (r, cases[h].id), uh.margin_for(cases[h], "probs"))
    for r in INVALID:
        assert bool(torch.isnan(probs[r]).all().cpu()), r
    for r in DISABLED:
        assert bool((probs[r] == CANARY).all().cpu()), r
    assert bool((buf[:PAD] == CANARY).all().cpu()) and bool((buf[PAD + R:] == CANARY).all().cpu())
    # routes of one head on several slots differ (the slots' rows do), routes of several heads on one slot differ (the heads do)
    assert not torch.equal(probs[0], probs[1]) and not torch.equal(probs[3], probs[4])
    group.close()


def test_a_route_whose_rows_pass_the_batch_is_invalid_and_reads_nothing_past_it():
    """The embedding one row short of what the last slot needs: the two routes of the last slot join the invalid ones, the others stand."""
    import torch
    rows = 3
    cases, heads, group, emb, d_slot, d_head = _setup(64, 18, rows)
    probs, invalid = group.forward_routes(emb[:SLOTS * rows - 1], d_slot, d_head, rows, SLOTS)
    last = [r for r in VALID if ROUTES[r][0] == SLOTS - 1]
    assert len(last) == 2 and int(invalid.cpu()[0]) == len(INVALID) + 2
    for r in VALID:
        s, h = ROUTES[r]
        if r in last:
            assert bool(torch.isnan(probs[r]).all().cpu())
        else:
            assert torch.equal(probs[r], heads[h].forward(emb[s * rows:(s + 1) * rows]))
    group.close()


def test_the_tables_are_read_by_the_kernel_so_a_captured_call_follows_their_edits():
    import torch
    rows = 3
    cases, heads, group, emb, d_slot, d_head = _setup(64, 18, rows)
    R = len(ROUTES)
    out = torch.zeros((R, rows, CLASSES), dtype=torch.float32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        group.forward_routes(emb, d_slot, d_head, rows, SLOTS, out=out, invalid=bad)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        group.forward_routes(emb, d_slot, d_head, rows, SLOTS, out=out, invalid=bad)
    out.fill_(CANARY)
    d_slot[7], d_head[7] = 3, 5                                              # the disabled route attached; an invalid one repaired
    d_head[9] = 0
    g.replay()
    assert int(bad.cpu()[0]) == len(INVALID) - 1
    assert torch.equal(out[7], heads[5].forward(emb[3 * rows:4 * rows])) and torch.equal(out[9], heads[0].forward(emb[rows:2 * rows]))
    assert torch.equal(out[0], heads[2].forward(emb[:rows]))
    group.close()


def test_no_routes_or_no_rows_launch_nothing_and_dimensions_off_the_matrix_cores_are_unsupported():
    import torch
    from multilingual_kws_amd.head import Head, HeadGroup
    cases, heads, group, emb, d_slot, d_head = _setup(64, 18, 3)
    L, s = _lib.lib(), _lib.current_stream_ptr()
    out = torch.full((len(ROUTES), 3, CLASSES), CANARY, dtype=torch.float32, device="cuda")
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    call = lambda g=group.h, e=emb.data_ptr(), B=15, rows=3, n_slots=SLOTS, rs=d_slot.data_ptr(), rh=d_head.data_ptr(), n=len(ROUTES), o=out.data_ptr(), \
        b=bad.data_ptr(): L.mkws_head_group_forward_routes(g, e, B, rows, n_slots, rs, rh, n, o, b, s)
    assert call(n=0) == 0 and call(rows=0) == 0 and call(n=0, e=None, rs=None, rh=None, o=None, b=None) == 0
    torch.cuda.synchronize()
    assert int(bad.cpu()[0]) == 77 and bool((out == CANARY).all().cpu())    # nothing launched, nothing written
    probs, invalid = group.forward_routes(emb, d_slot[:0], d_head[:0], 3, SLOTS)
    assert tuple(probs.shape) == (0, 3, CLASSES)
    for kw in (dict(g=None), dict(B=-1), dict(rows=-1), dict(n_slots=-1), dict(n=-1), dict(e=None), dict(rs=None), dict(rh=None), dict(o=None), dict(b=None)):
        assert call(**kw) == -1, kw
    assert call() == 0
    for dims in ((24, 18), (64, 40)):
        if dims[1] > 32:                                                    # (a head wider than 32 cannot be created at all)
            with pytest.raises(_lib.MkwsError) as ei:
                Head(dims[0], dims[1], CLASSES, max_batch=16)
            assert ei.value.code == -2
            continue
        odd = HeadGroup([Head(dims[0], dims[1], CLASSES, max_batch=16, seed=k) for k in range(2)])
        x = torch.zeros((15, dims[0]), dtype=torch.float32, device="cuda")
        with pytest.raises(_lib.MkwsError) as ei:
            odd.forward_routes(x, d_slot, d_head, 3, SLOTS)
        assert ei.value.code == -2
        assert call(g=odd.h, e=x.data_ptr()) == -2 and call(g=odd.h, e=x.data_ptr(), n=0) == -2      # refused before the empty call returns
        odd.close()
    group.close()
