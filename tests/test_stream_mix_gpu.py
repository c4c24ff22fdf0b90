"""mkws_stream_mix / mkws_stream_power / mkws_stream_bed_gain on the device against the position-by-position restatement of
tests/util_compose.py: byte for byte, over an output pre-filled with a canary that must survive everywhere outside the valid streams."""
import ctypes
import math

import numpy as np
import pytest

from multilingual_kws_amd import _lib, compose
from tests import util_compose as uc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(c, src=None):
    """One launch of a case over a canary-filled output -> (the output on the host, the invalid count)."""
    import torch
    d_src = torch.from_numpy(c.src).cuda() if src is None else src
    out = torch.full((c.out_floats,), float(uc.CANARY), dtype=torch.float32, device="cuda")
    gains = None if c.bed_gain is None else torch.from_numpy(c.bed_gain).cuda()
    out, bad = compose.mix_on_device(d_src, c.items, c.descs, gains, c.clip, out=out, max_out=c.max_out, validate=False, check=False)
    return out.cpu().numpy(), int(bad.cpu()[0])


@pytest.mark.parametrize("maker", uc.CASES, ids=lambda m: m.__name__[5:])
def test_mix_equals_the_restatement(maker):
    c = uc.get(maker)
    want, _ = c.expected
    got, bad = _run(c)
    assert bad == 0
    differ = np.nonzero(_bits(got) != _bits(want))[0]
    assert differ.size == 0, (differ[:8], got[differ[:8]], want[differ[:8]])


def test_invalid_tables_are_counted_and_skipped():
    c = uc.get(uc.case_invalid)
    want, want_bad = c.expected
    assert want_bad >= len(uc.BAD_ITEMS) + len(uc.BAD_STREAMS)
    got, bad = _run(c)
    assert bad == want_bad
    assert np.array_equal(_bits(got), _bits(want))
    # the untouched neighbours were written, the refused streams kept their canary
    first, spoilt = c.desc_rows[0], c.desc_rows[len(uc.BAD_ITEMS) + 1]
    assert not np.any(got[first["out_offset"]:first["out_offset"] + first["n_out"]] == uc.CANARY)
    assert np.all(got[spoilt["out_offset"]:spoilt["out_offset"] + uc.INVALID_N_OUT] == uc.CANARY)
    # the wrapper raises on the count when asked to check, and refuses on the host before anything runs when asked to validate
    import torch
    with pytest.raises(ValueError, match=f"refused {want_bad} of"):
        compose.mix_on_device(torch.from_numpy(c.src).cuda(), c.items, c.descs, out_floats=c.out_floats, max_out=c.max_out, validate=False)
    with pytest.raises(ValueError, match="stream item"):
        compose.mix_on_device(torch.from_numpy(c.src).cuda(), c.items, c.descs, out_floats=c.out_floats, max_out=c.max_out)
    # the power launch counts the same items and streams (all but the one whose output does not fit, which it never writes)
    _, bad_p = compose.power_on_device(torch.from_numpy(c.src).cuda(), c.items, c.descs, max_out=c.max_out, validate=False, check=False)
    assert int(bad_p.cpu()[0]) == want_bad - 1


def test_nothing_to_do_and_bad_arguments():
    import torch
    L = _lib.lib()
    c = uc.get(uc.case_lengths)
    src = torch.from_numpy(c.src).cuda()
    out = torch.full((64,), float(uc.CANARY), dtype=torch.float32, device="cuda")
    invalid = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    keep, p_items, p_descs = compose.upload_tables(c.items, c.descs, src.device)
    P, st = ctypes.c_void_p, _lib.current_stream_ptr()

    def mix(n_streams, max_out, src_floats=src.numel(), descs=p_descs, out_floats=64, bad=invalid.data_ptr()):
        return L.mkws_stream_mix(P(src.data_ptr()), src_floats, P(p_items), len(c.items), P(descs), n_streams, None, 1, max_out, P(out.data_ptr()),
                                 out_floats, P(bad), st)

    assert mix(0, 4099) == 0 and mix(len(c.descs), 0) == 0
    partials = torch.full((8,), 5.0, dtype=torch.float64, device="cuda")
    assert L.mkws_stream_power(P(src.data_ptr()), src.numel(), P(p_items), len(c.items), P(p_descs), 0, 4099, P(partials.data_ptr()),
                               P(invalid.data_ptr()), st) == 0
    assert L.mkws_stream_bed_gain(P(partials.data_ptr()), P(p_descs), len(c.descs), 0, P(partials.data_ptr()), P(out.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert int(invalid.cpu()[0]) == 77 and bool((out == float(uc.CANARY)).all().cpu()) and bool((partials == 5.0).all().cpu())
    assert mix(-1, 10) == -1 and mix(1, -1) == -1 and mix(1, 10, src_floats=-1) == -1 and mix(1, 10, out_floats=-1) == -1
    assert mix(1, 10, descs=None) == -1 and mix(1, 10, bad=None) == -1
    assert b"NULL" in L.mkws_last_error()
    assert mix(3, 1 << 41) == -2 and b"exceed one launch" in L.mkws_last_error()             # MKWS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(invalid.cpu()[0]) == 77 and bool((out == float(uc.CANARY)).all().cpu())


def test_offsets_above_2_to_31():
    """A source offset and an output offset above 2^31 floats: an index cut to 32 bits would land in the low regions, which hold
    other audio (source) and must keep their canary (output).  Only the touched ranges of the big buffers are initialised."""
    import torch
    big = 1 << 31
    small = uc.Case("small", np.concatenate([uc._noise(2200, 20), uc._noise(700, 21)]),
                    *uc.layout([dict(n_out=2300, off=1, items=[uc.item(5, 2100, -3, 2100, 7, 40, 40, 0.8), uc.item(5, 2100, 100, 900, 1500)],
                                     bed=(2200, 700, 699))]), bed_gain=[0.3])
    want, _ = small.expected
    src = torch.empty(big + 4096, dtype=torch.float32, device="cuda")
    src[:2900] = 0.75                                                         # what an index cut to 31 bits would read
    base = big + 1000                                                         # a multiple of four floats: the case keeps its alignment
    src[base:base + 2900] = torch.from_numpy(small.src).cuda()
    out = torch.empty(big + 4096, dtype=torch.float32, device="cuda")
    out[:4096] = float(uc.CANARY)
    out[big:] = float(uc.CANARY)
    items, descs = small.items.copy(), small.descs.copy()
    items["src_offset"] += base
    descs["bed_offset"] += base
    descs["out_offset"] += base
    compose.mix_on_device(src, items, descs, torch.from_numpy(small.bed_gain).cuda(), True, out=out)
    assert bool((out[:4096] == float(uc.CANARY)).all().cpu())
    got = out[base:base + small.out_floats].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert bool((out[big:base] == float(uc.CANARY)).all().cpu())
    del src, out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------
# signal-to-noise ratio
# ---------------------------------------------------------------------------------------------------
SNR_N_OUT = (1, 1024, 1025, 50000)
SNR_DB = (-10.0, 0.0, 10.0, 30.0)


def _snr_case():
    """One stream per (n_out, snr): two overlapping items over a bed of 777 samples; then a silent foreground and a silent bed."""
    src = np.concatenate([uc._noise(30000, 30) * np.float32(0.5), uc._noise(777, 31) * np.float32(0.2), np.zeros(100, np.float32)])
    streams = []
    for n in SNR_N_OUT:
        for _ in SNR_DB:
            streams.append(dict(n_out=n, off=len(streams) % 4, bed=(30000, 777, 5),
                                items=[uc.item(0, 30000, 11, min(n, 30000), 0, 0, 0, 0.5), uc.item(0, 30000, 0, min(n, 27000), n // 2, 10, 10)]))
    streams.append(dict(n_out=1500, off=0, bed=(30000, 777, 0), items=[uc.item(30777, 100, 0, 100, 3)]))         # a silent foreground
    streams.append(dict(n_out=1500, off=0, bed=(30777, 100, 0), items=[uc.item(0, 30000, 0, 1500, 0)]))          # a silent bed
    streams.append(dict(n_out=1500, off=0, bed=None, items=[uc.item(0, 30000, 0, 1500, 0)]))                     # no bed
    snr = list(SNR_DB) * len(SNR_N_OUT) + [10.0, 10.0, 10.0]
    return uc.Case("snr", src, *uc.layout(streams)), snr


def test_snr_gain_and_mix():
    import torch
    c, snr = _snr_case()
    src = torch.from_numpy(c.src).cuda()
    tables = compose.upload_tables(c.items, c.descs, src.device)
    partials = compose.power_on_device(src, c.items, c.descs, tables=tables)
    again = compose.power_on_device(src, c.items, c.descs, tables=tables)
    assert partials.shape == (len(c.descs), compose.n_tiles(50000), 2)
    assert torch.equal(partials.view(torch.int64), again.view(torch.int64)), "two launches gave different partials"
    gains = compose.bed_gain_on_device(partials, c.descs, compose.snr_scale(snr), tables=tables).cpu().numpy()
    # against float64 fsum powers: the correctly rounded float32 or its neighbour (a relative 2^-22)
    p_fg, p_bed = c.powers()
    host = compose.bed_gain_host(*compose.power_host(c.src, c.items, c.descs), c.descs, compose.snr_scale(snr))
    for r in range(len(c.descs)):
        want = uc.gain_for(p_fg[r], p_bed[r], c.desc_rows[r]["bed_len"] > 0, snr[r])
        print(f"stream {r}: n_out {c.desc_rows[r]['n_out']}, snr {snr[r]}: device gain {gains[r]!r}, float64 {want!r}, bed_gain_host {host[r]!r}")
        assert abs(float(gains[r]) - want) <= 2.0 ** -22 * want, (r, gains[r], want)
        assert abs(float(gains[r]) - float(host[r])) <= 2.0 ** -22 * want, (r, gains[r], host[r])
    assert gains[-3:].tolist() == [0.0, 0.0, 0.0] and np.all(gains[:-3] > 0)
    # the sums of the partials are the float64 powers up to reordering
    sums = partials.cpu().numpy().sum(axis=1)
    assert np.allclose(sums[:, 0], p_fg, rtol=1e-12, atol=0) and np.allclose(sums[:, 1], p_bed, rtol=1e-12, atol=0)
    # the audio: bit-equal to the restatement fed the device's own gains, and at the wanted ratio
    mixed = uc.Case("snr_mixed", c.src, c.item_rows, c.desc_rows, bed_gain=gains, clip=True, cache=c.cache)
    want, _ = mixed.expected
    got, bad = _run(mixed, src)
    assert bad == 0 and np.array_equal(_bits(got), _bits(want))
    for r in range(len(c.descs) - 3):
        ratio = 10 * math.log10(p_fg[r] / (float(gains[r]) ** 2 * p_bed[r]))
        assert abs(ratio - snr[r]) < 1e-5, (r, ratio)


def test_power_gain_mix_in_one_graph():
    """power -> bed_gain -> mix captured as one chain (no parallel branches) and replayed on changed source audio."""
    import torch
    src_np = np.concatenate([uc._noise(5000, 40) * np.float32(0.4), uc._noise(900, 41) * np.float32(0.3)])
    items, descs = uc.layout([dict(n_out=4099, off=1, bed=(5000, 900, 17), items=[uc.item(0, 5000, 0, 3000, 0, 0, 100), uc.item(0, 5000, 2000, 1300, 2900, 100, 0)]),
                              dict(n_out=1025, off=3, bed=(5000, 900, 899), items=[uc.item(0, 5000, 100, 1000, 20)])])
    c = uc.Case("graph", src_np, items, descs)
    src = torch.from_numpy(c.src).cuda()
    tables = compose.upload_tables(c.items, c.descs, src.device)
    scale = torch.from_numpy(compose.snr_scale([10.0, 0.0])).cuda()
    partials = torch.zeros((2, compose.n_tiles(c.max_out), 2), dtype=torch.float64, device="cuda")
    gains = torch.zeros(2, dtype=torch.float32, device="cuda")
    out = torch.full((c.out_floats,), float(uc.CANARY), dtype=torch.float32, device="cuda")

    def chain():
        compose.power_on_device(src, c.items, c.descs, partials=partials, validate=False, check=False, tables=tables)
        compose.bed_gain_on_device(partials, c.descs, scale, bed_gain=gains, tables=tables)
        compose.mix_on_device(src, c.items, c.descs, gains, True, out=out, validate=False, check=False, tables=tables)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for seed in (50, 51):
        new = np.concatenate([uc._noise(5000, seed) * np.float32(0.4), uc._noise(900, seed + 10) * np.float32(0.3)])
        src.copy_(torch.from_numpy(new).cuda())
        out.fill_(float(uc.CANARY))
        graph.replay()
        torch.cuda.synchronize()
        g = gains.cpu().numpy()
        p_fg, p_bed = uc.powers(new, c.item_rows, c.desc_rows, c.max_out)
        for r, snr in enumerate((10.0, 0.0)):
            want = uc.gain_for(p_fg[r], p_bed[r], True, snr)
            assert abs(float(g[r]) - want) <= 2.0 ** -22 * want
        want_audio, _ = uc.Case("graph_replay", new, c.item_rows, c.desc_rows, bed_gain=g).expected
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want_audio))
