"""mkws_head_group_forward_segments / HeadGroup.forward_segments: every row of a concatenation of segments under the head of its own
segment.  The yardstick is Head.forward on each segment's rows alone and the comparison is torch.equal: the segmented kernel runs the
single-head kernel's own K walk and epilogue per (tile, segment), so there is no tolerance to choose."""
import numpy as np
import pytest

LENGTHS = [1, 0, 15, 16, 17, 0, 33]          # one-row and empty segments, tiles that straddle two and three segments, more than one tile
HEADS = [2, 0, 1, 1, 0, 2, 1]
ROWS = sum(LENGTHS)                          # 82: six 16-row tiles, the last with two rows
DIMS = [(32, 18, 3), (1024, 8, 3)]           # NT = 2 (hidden > 16) and NT = 1
SENTINEL = -7.0
PAD = 3                                      # canary rows on both sides of the output


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: f"in{d[0]}_hid{d[1]}")
def setup(request):
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.head import Head, HeadGroup, glorot_uniform_params
    in_dim, hid, cls = request.param
    heads = [Head(in_dim, hid, cls, max_batch=128, params=glorot_uniform_params(in_dim, hid, cls, seed=40 + k)) for k in range(3)]
    group = HeadGroup(heads)
    emb = torch.from_numpy(np.random.default_rng(in_dim).standard_normal((ROWS, in_dim)).astype(np.float32)).cuda()
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    # the reference, once: each segment's rows through its own head alone
    want = torch.full((ROWS, cls), float("nan"), device="cuda")
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if b > a:
            want[a:b] = heads[HEADS[s]].forward(emb[a:b])
    assert not torch.isnan(want).any()
    assert not torch.equal(heads[0].forward(emb), heads[1].forward(emb))                 # the heads differ: a wrong head would show
    yield dict(torch=torch, heads=heads, group=group, emb=emb, off=off, want=want, cls=cls)
    group.close()


def _call(su, off, seg_head, batches=((0, ROWS),)):
    """-> (padded output, rows [PAD, PAD + ROWS) being the rows of the concatenation; total of the invalid counters)."""
    torch = su["torch"]
    out = torch.full((ROWS + 2 * PAD, su["cls"]), SENTINEL, device="cuda")
    d_off = torch.from_numpy(np.asarray(off, np.int32)).cuda()
    d_head = torch.from_numpy(np.asarray(seg_head, np.int32)).cuda()
    bad = 0
    for r0, n in batches:
        probs, invalid = su["group"].forward_segments(su["emb"][r0:r0 + n], d_off, d_head, row_base=r0, out=out[PAD + r0:PAD + r0 + n])
        assert probs.data_ptr() == out[PAD + r0:].data_ptr()
        bad += int(invalid.cpu()[0])
    return out, bad


@pytest.mark.gpu
@pytest.mark.parametrize("batches", [((0, ROWS),), ((0, 7), (7, 40), (47, 35))], ids=["one_call", "batches_7_40_35"])
def test_every_row_equals_its_own_heads_forward_bit_for_bit(setup, batches):
    torch = setup["torch"]
    out, bad = _call(setup, setup["off"], HEADS, batches)
    assert bad == 0
    assert torch.equal(out[PAD:PAD + ROWS], setup["want"])
    assert bool((out[:PAD] == SENTINEL).all()) and bool((out[PAD + ROWS:] == SENTINEL).all())          # canaries


@pytest.mark.gpu
def test_rows_outside_the_batch_are_untouched(setup):
    torch = setup["torch"]
    out, bad = _call(setup, setup["off"], HEADS, ((7, 40),))
    assert bad == 0 and torch.equal(out[PAD + 7:PAD + 47], setup["want"][7:47])
    assert bool((out[:PAD + 7] == SENTINEL).all()) and bool((out[PAD + 47:] == SENTINEL).all())


@pytest.mark.gpu
def test_a_head_index_outside_the_group_gives_nan_rows_for_exactly_its_segments(setup):
    torch = setup["torch"]
    seg_head = list(HEADS)
    seg_head[2], seg_head[4] = -1, 3                                                               # rows 1..16 and 32..49
    out, bad = _call(setup, setup["off"], seg_head)
    got, want, off = out[PAD:PAD + ROWS], setup["want"], setup["off"]
    nan_rows = torch.isnan(got).all(dim=1)
    assert nan_rows.nonzero().flatten().tolist() == list(range(off[2], off[3])) + list(range(off[4], off[5]))
    assert bad == LENGTHS[2] + LENGTHS[4]
    assert torch.equal(got[~nan_rows], want[~nan_rows]) and not torch.isnan(got[~nan_rows]).any()  # the neighbours are unchanged
    assert bool((out[:PAD] == SENTINEL).all()) and bool((out[PAD + ROWS:] == SENTINEL).all())


@pytest.mark.gpu
def test_rows_that_no_segment_covers_are_nan_and_counted(setup):
    torch = setup["torch"]
    off = setup["off"].copy()
    off[-1] -= 5                                                                                   # the last 5 rows belong to nobody
    out, bad = _call(setup, off, HEADS)
    got = out[PAD:PAD + ROWS]
    assert bad == 5 and bool(torch.isnan(got[ROWS - 5:]).all())
    assert torch.equal(got[:ROWS - 5], setup["want"][:ROWS - 5])
    # the same through batches: the counter is per call
    out2, bad2 = _call(setup, off, HEADS, ((0, 7), (7, 40), (47, 35)))
    assert bad2 == 5 and torch.equal(out2.nan_to_num(nan=-1.0), out.nan_to_num(nan=-1.0))
    # an empty call launches nothing and writes nothing
    probs, invalid = setup["group"].forward_segments(setup["emb"][:0], torch.from_numpy(off).cuda(), torch.tensor(HEADS, dtype=torch.int32, device="cuda"))
    assert tuple(probs.shape) == (0, setup["cls"]) and int(invalid.cpu()[0]) == 0


@pytest.mark.gpu
def test_dimensions_off_the_matrix_core_path_are_unsupported_and_bad_arguments_refused():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.head import Head, HeadGroup
    heads = [Head(20, 18, 3, max_batch=16, seed=k) for k in range(2)]
    group = HeadGroup(heads)
    emb = torch.zeros((4, 20), device="cuda")
    off, sh = torch.tensor([0, 4], dtype=torch.int32, device="cuda"), torch.tensor([0], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.MkwsError) as e:
        group.forward_segments(emb, off, sh)
    assert e.value.code == -2                                                                      # MKWS_ERR_UNSUPPORTED
    group.close()
    ok = HeadGroup([Head(32, 18, 3, max_batch=16, seed=0)])
    emb = torch.zeros((4, 32), device="cuda")
    L, out, bad = _lib.lib(), torch.zeros((4, 3), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    s = _lib.current_stream_ptr()
    assert L.mkws_head_group_forward_segments(None, emb.data_ptr(), 4, 0, off.data_ptr(), sh.data_ptr(), 1, out.data_ptr(), bad.data_ptr(), s) == -1
    assert L.mkws_head_group_forward_segments(ok.h, emb.data_ptr(), -1, 0, off.data_ptr(), sh.data_ptr(), 1, out.data_ptr(), bad.data_ptr(), s) == -1
    assert L.mkws_head_group_forward_segments(ok.h, emb.data_ptr(), 4, -1, off.data_ptr(), sh.data_ptr(), 1, out.data_ptr(), bad.data_ptr(), s) == -1
    assert L.mkws_head_group_forward_segments(ok.h, emb.data_ptr(), 4, 0, None, sh.data_ptr(), 1, out.data_ptr(), bad.data_ptr(), s) == -1
    assert L.mkws_head_group_forward_segments(ok.h, emb.data_ptr(), 4, 0, off.data_ptr(), sh.data_ptr(), 1, out.data_ptr(), None, s) == -1
    assert L.mkws_head_group_forward_segments(ok.h, None, 0, 0, None, None, 1, None, None, s) == 0            # B == 0: nothing to do
    assert L.mkws_head_group_forward_segments(ok.h, emb.data_ptr(), 4, 0, off.data_ptr(), sh.data_ptr(), 0, out.data_ptr(), bad.data_ptr(), s) == 0
    with pytest.raises(ValueError):
        ok.forward_segments(emb, off, torch.tensor([0, 0], dtype=torch.int32, device="cuda"))      # 2 offsets for 2 segments
    with pytest.raises(ValueError):
        ok.forward_segments(emb, off.to(torch.int64), sh)
    ok.close()


@pytest.mark.gpu
def test_the_call_is_capturable(setup):
    torch = setup["torch"]
    from multilingual_kws_amd import _lib
    L, g, emb = _lib.lib(), setup["group"], setup["emb"]
    d_off, d_head = torch.from_numpy(setup["off"]).cuda(), torch.tensor(HEADS, dtype=torch.int32, device="cuda")
    static_in = emb.clone()
    out = torch.full((ROWS, setup["cls"]), SENTINEL, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")

    def chain():
        assert L.mkws_head_group_forward_segments(g.h, static_in.data_ptr(), ROWS, 0, d_off.data_ptr(), d_head.data_ptr(), len(HEADS), out.data_ptr(),
                                                  bad.data_ptr(), _lib.current_stream_ptr()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    seen = []
    for _ in range(2):
        out.fill_(SENTINEL)
        bad.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(bad.cpu()[0]) == 0
        seen.append(out.clone())
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], setup["want"])
    static_in.copy_(emb.flip(0))                                                                   # the replay reads the static input anew
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, setup["want"]) and not torch.isnan(out).any()
