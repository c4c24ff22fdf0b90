"""The live form of the resampler (mkws_resample_live_push_many) against its specification -- the pushes of a stream, concatenated, are the
first samples of mkws_resample_forward(centred = 0) over the stream's whole input, bit for bit -- and the live sessions fed at another rate
than the model's against the same sessions fed the converted audio."""
import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from multilingual_kws_amd.resample import Resampler
from tests.util_resample import noise_f32, noise_i16

pytestmark = pytest.mark.gpu
RATES = (48000, 44100, 8000)
THRESHOLDS = (0.2, 0.5, 0.8)
HOP = 320


@pytest.fixture(scope="module")
def handles():
    hs = {r: Resampler(r) for r in RATES}
    yield hs
    for h in hs.values():
        h.close()


def _push_all(rs, x, out_samples, states=None):
    """x: CUDA [n] (float32 or int16) pushed whole -> the concatenated outputs."""
    import torch
    n_in = rs.live_in_samples(out_samples)
    states = rs.live_state_many(1) if states is None else states
    rows = [rs.live_push_many(states, x[None, i * n_in:(i + 1) * n_in].contiguous(), out_samples)[0] for i in range(x.numel() // n_in)]
    return torch.cat(rows), states


@pytest.mark.parametrize("rate", RATES)
def test_chunking_does_not_matter(handles, rate):
    """Two seconds in pushes of one hop and of four (more than one tile of the kernel), float32, int16 and int16's values as float32."""
    import torch
    rs = handles[rate]
    x = torch.from_numpy(noise_f32(2 * rate, rate)).cuda()
    pcm = torch.from_numpy(noise_i16(2 * rate, rate + 1)).cuda()
    want, want_pcm = rs.forward(x, centred=False), rs.forward(pcm, centred=False)
    assert want.numel() == 32000
    for out_samples in (HOP, 4 * HOP):
        got, state = _push_all(rs, x, out_samples)
        assert torch.equal(got, want) and int(state[0, 0].cpu()) == 2 * rate
        assert torch.equal(_push_all(rs, pcm, out_samples)[0], want_pcm)
        assert torch.equal(_push_all(rs, pcm.to(torch.float32) / 32768.0, out_samples)[0], want_pcm)


def test_three_streams_with_a_changing_mask(handles):
    """Streams at different positions, an active mask that changes with every push: an active stream gets the next samples of its own
    causal output, an inactive one keeps its state bytes and its output row; a slice pushed alone equals the slice pushed in place."""
    import torch
    rs = handles[44100]
    n_in, S, GUARD = rs.live_in_samples(HOP), 3, 777.0
    xs = [torch.from_numpy(noise_f32(40 * n_in, 30 + s)).cuda() for s in range(S)]
    want = [rs.forward(x, centred=False) for x in xs]
    states, alone = rs.live_state_many(S), rs.live_state_many(S)
    at = [0] * S
    for i in range(45):
        on = [int(i % 2 == 0 or i > 20), int(i % 3 != 1), int(i >= 7)]
        on = [o and at[s] < 40 for s, o in enumerate(on)]
        if not any(on):
            continue
        audio = torch.stack([xs[s][min(at[s], 39) * n_in:(min(at[s], 39) + 1) * n_in] for s in range(S)])
        before = states.clone()
        out = torch.full((S, HOP), GUARD, device="cuda")
        rs.live_push_many(states, audio, HOP, active=torch.tensor(on, dtype=torch.int32, device="cuda"), out=out)
        for s in range(S):
            if on[s]:
                assert torch.equal(out[s], want[s][at[s] * HOP:(at[s] + 1) * HOP]), (i, s)
                one = alone[s:s + 1].clone()                       # the slice copied out, pushed alone, copied back
                got = rs.live_push_many(one, audio[s:s + 1].contiguous(), HOP)
                alone[s].copy_(one[0])
                assert torch.equal(got[0], out[s]) and torch.equal(alone[s], states[s])
                at[s] += 1
                assert int(states[s, 0].cpu()) == at[s] * n_in
            else:
                assert torch.equal(states[s], before[s]) and bool((out[s] == GUARD).all())
    assert at == [35, 30, 38]


def test_snapshot_restore_and_reset(handles):
    import torch
    rs = handles[8000]
    n_in = rs.live_in_samples(HOP)
    x = torch.from_numpy(noise_f32(30 * n_in, 4)).cuda()
    first, state = _push_all(rs, x[:10 * n_in], HOP)
    snap = state.clone()
    rest, _ = _push_all(rs, x[10 * n_in:], HOP, state)
    assert torch.equal(torch.cat([first, rest]), rs.forward(x, centred=False))
    state.copy_(snap)                                                # restore: the replay is identical
    assert torch.equal(_push_all(rs, x[10 * n_in:], HOP, state)[0], rest)
    state.zero_()                                                    # reset: a zero block is a fresh stream
    assert torch.equal(_push_all(rs, x[:10 * n_in], HOP, state)[0], first)


@pytest.mark.parametrize("rate,out_samples", [(48000, 20), (8000, 32)])
def test_pushes_shorter_than_the_history(handles, rate, out_samples):
    """A push of fewer input samples than the T - 1 the state keeps: part of the new history is the old one, moved down."""
    import torch
    rs = handles[rate]
    n_in = rs.live_in_samples(out_samples)
    assert n_in < rs.geometry["T"] - 1
    x = torch.from_numpy(noise_f32(40 * n_in, rate + 7)).cuda()
    got, state = _push_all(rs, x, out_samples)
    assert torch.equal(got, rs.forward(x, centred=False)[:40 * out_samples]) and int(state[0, 0].cpu()) == 40 * n_in
    # the history the short pushes left is the one a single long push leaves
    one = rs.live_state_many(1)
    rs.live_push_many(one, x[None].contiguous(), 40 * out_samples)
    assert torch.equal(one, state)


def test_a_captured_push_advances_the_streams(handles):
    import torch
    rs = handles[48000]
    n_in, S = rs.live_in_samples(HOP), 2
    xs = torch.from_numpy(np.stack([noise_f32(6 * n_in, 50 + s) for s in range(S)])).cuda()
    states, audio, out = rs.live_state_many(S), torch.zeros((S, n_in), device="cuda"), torch.zeros((S, HOP), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rs.live_push_many(states, audio, HOP, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rs.live_push_many(states, audio, HOP, out=out)
    states.zero_()
    eager_states, rows = rs.live_state_many(S), []
    for i in range(6):
        audio.copy_(xs[:, i * n_in:(i + 1) * n_in])
        g.replay()
        assert torch.equal(out, rs.live_push_many(eager_states, xs[:, i * n_in:(i + 1) * n_in].contiguous(), HOP)), i
        rows.append(out.clone())
    assert torch.equal(states, eager_states) and states[:, 0].tolist() == [6 * n_in] * S
    assert torch.equal(torch.cat(rows, dim=1), rs.forward(xs, centred=False))


# -- the sessions ----------------------------------------------------------------------------------------------------------------------

def _speechlike(rate, seconds, seed):
    """Tones that move every quarter of a second over a little noise, float32 at `rate`."""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / rate
    f = 400.0 + 300.0 * ((np.arange(n) // (rate // 4) + seed) % 4)
    return (0.4 * np.sin(2 * np.pi * f * t) + 0.02 * rng.standard_normal(n)).astype(np.float32)


def _models(max_batch):
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=max_batch)
    return [tl.TransferLearnedModel(emb, Head(max_batch=max_batch, seed=s), blob, "synthetic") for s in (1, 2, 3)]


def _session_against_converted(rate, push, hops, delay_ms):
    """LiveSession(input_rate=rate, hops_per_push=hops) fed audio at `rate` in ragged chunks = the session without input_rate, on the same
    handle, fed the causal conversion of the same audio: the same rows, the same records (scores bit-equal)."""
    models = _models(hops)
    x = _speechlike(rate, 2.0, 3)
    first = 5 * push
    x[:first] = (np.round(x[:first] * 32768) / 32768).astype(np.float32)     # the first chunk is also fed as int16 PCM
    rs = Resampler(rate)
    y = rs.forward(x, centred=False)
    assert y.shape == (32000,)
    plain = bsa.LiveSession(models, THRESHOLDS, fired_only=False, hops_per_push=hops)
    assert not hasattr(plain, "resampler")
    want_rows, want_records = [], []
    for at in range(0, y.size, 1280):
        want_rows += plain.feed(y[at:at + 1280])
        want_records += plain.last_records
    assert plain.windows_seen == 51 and len(want_records) >= 3
    sess = bsa.LiveSession(models, THRESHOLDS, fired_only=False, input_rate=rate, hops_per_push=hops)
    assert sess.resampler.delay_ms == delay_ms and sess.graph is not None
    assert sess.in_push_samples == push and sess.push_samples == HOP * hops
    import torch
    for as_i16 in (False, True):
        rows, records, at = [], [], 0
        sizes = [first, 1, push - 1, push, 12 * push + 825, 7, 31 * push + 240]
        k = 0
        while at < x.size:
            n = sizes[k % len(sizes)]
            chunk = x[at:at + n]
            if as_i16 and at == 0:
                chunk = np.round(chunk * 32768).astype(np.int16)
            elif k % 3 == 2:
                chunk = torch.from_numpy(chunk).cuda()
            rows += sess.feed(chunk)
            records += sess.last_records
            at += n
            k += 1
            assert sess.samples_seen == min(at, x.size)
            assert sess.windows_seen == max(0, (min(at, x.size) // push * HOP * hops - 16000) // 320 + 1)
        assert rows == want_rows and records == want_records
        assert sess.windows_seen == 51 and sess.samples_seen == 2 * rate
        sess.reset()
        assert sess.samples_seen == 0 and not bool(sess.rstate.any().cpu())
    for s in (sess, plain):
        s.close()
    rs.close()


@pytest.mark.parametrize("rate,push", [(48000, 960), (22050, 441), (96000, 1920)])
def test_live_session_at_48k(rate, push):
    """At 48 kHz (chunks of 4800, 1, 959, 960, 12345, 7 and 30000 samples), at 22 050 Hz (L = 320) and at 96 kHz (a history of 384
    samples, longer than the resampler's workgroup)."""
    _session_against_converted(rate, push, 1, 2.0)


def test_live_session_at_11025_with_two_hops_per_push():
    """The session the refusal of LiveSession(input_rate=11025) recommends (test_live_session_input_rate_of_the_model_changes_nothing):
    hops_per_push=2, pushes of 441 samples for 640; the delay is 32 / 11025 s, half / (L * rate_in)."""
    _session_against_converted(11025, 441, 2, 1000.0 * 20480 / (640 * 11025))


@pytest.mark.parametrize("rate", [22050, 96000])
def test_read_wav_at_other_rates(rate, tmp_path):
    """input_data.read_wav_at on a WAV at `rate` = Resampler(rate).forward(centred=True) over the decoded file, which
    tests/test_resample_geometries_gpu.py holds to the emulator."""
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import input_data
    pcm = np.round(_speechlike(rate, 0.5, 8) * 20000).astype(np.int16)
    path = str(tmp_path / f"clip_{rate}.wav")
    with open(path, "wb") as fh:
        fh.write(synth.wav_bytes(pcm, rate=rate))
    with open(path, "rb") as fh:
        x, got_rate = input_data.decode_wav(fh.read())
    assert got_rate == rate and np.array_equal(x, pcm.astype(np.float32) / np.float32(32768))
    rs = Resampler(rate)
    want = rs.forward(x, centred=True)
    assert want.shape == (8000,) and want.dtype == np.float32 and np.abs(want).max() > 0.1
    assert np.array_equal(want.view(np.uint32), rs.forward(pcm, centred=True).view(np.uint32))
    got = input_data.read_wav_at(path)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(input_data.read_wav_at(path, 16000, 9000)[:8000], want) and not input_data.read_wav_at(path, 16000, 9000)[8000:].any()
    rs.close()


def test_live_session_input_rate_of_the_model_changes_nothing():
    import torch
    models = _models(1)
    y = _speechlike(16000, 1.2, 5)
    a, b = bsa.LiveSession(models, THRESHOLDS), bsa.LiveSession(models, THRESHOLDS, input_rate=16000)
    assert not hasattr(a, "resampler") and not hasattr(b, "resampler") and b.in_push_samples == b.push_samples == 320
    assert a.feed(y) == b.feed(y) and a.last_records == b.last_records and torch.equal(a.probs, b.probs)
    assert a.samples_seen == b.samples_seen == y.size
    with pytest.raises(ValueError, match="hops_per_push that works is 2"):
        bsa.LiveSession(models, THRESHOLDS, input_rate=11025)
    a.close()
    b.close()


def test_live_group_at_44k1():
    """LiveSessionGroup(streams=3, input_rate=44100) against the group without input_rate fed, feed by feed, the converted samples of the
    pushes that feed completed (so that both run the same ticks): the same rows and records per slot."""
    S, PUSH = 3, 882
    models = _models(16)
    xs = [_speechlike(44100, 2.0, 11 + s) for s in range(S)]
    rs = Resampler(44100)
    ys = [rs.forward(x, centred=False) for x in xs]
    assert all(y.shape == (32000,) for y in ys)
    group = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, fired_only=False, input_rate=44100)
    plain = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, fired_only=False)
    assert group.in_push_samples == PUSH and group.resampler.delay_ms == 2.0 and not hasattr(plain, "resampler")
    with pytest.raises(ValueError, match="hops_per_push that works is 2"):
        bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, input_rate=11025)
    sizes = [(1000, 3333, 500), (882, 1, 4410), (2000, 1763, 1765)]
    at, n_records, i = [0] * S, 0, 0
    while min(at) < xs[0].size:
        fed = [s for s in range(S) if at[s] < xs[s].size and not (s == 1 and i < 4) and not (s == 2 and i % 2)]
        i += 1
        if not fed:
            continue
        chunks, same = {}, {}
        for s in fed:
            n = sizes[s][i % 3]
            chunks[s] = xs[s][at[s]:at[s] + n]
            done, at[s] = at[s] // PUSH, min(at[s] + n, xs[s].size)
            same[s] = ys[s][done * HOP:at[s] // PUSH * HOP]
        got, want = group.feed(chunks), plain.feed(same)
        assert got == want and group.last_records == plain.last_records, i
        n_records += sum(len(r) for r in group.last_records.values())
        for s in range(S):
            assert group.samples_seen(s) == at[s] and group.windows_seen(s) == plain.windows_seen(s)
    assert n_records >= 9 and [group.windows_seen(s) for s in range(S)] == [51] * S
    # reset(slot) restarts that slot's resampler only
    kept = group.rstates.clone()
    group.reset(1)
    assert not bool(group.rstates[1].any().cpu()) and group.samples_seen(1) == 0
    assert bool((group.rstates[0] == kept[0]).all().cpu()) and bool((group.rstates[2] == kept[2]).all().cpu()) and bool(kept[0].any().cpu())
    plain.reset(1)
    again = group.feed({1: xs[1][:20 * PUSH + 5]})
    assert again == plain.feed({1: ys[1][:20 * HOP]}) and group.samples_seen(1) == 20 * PUSH + 5
    for g in (group, plain):
        g.close()
    rs.close()


def test_live_routed_group_at_48k():
    """LiveRoutedGroup takes input_rate through LiveSessionGroup's slot buffers: two slots with their own routes, fed 48 kHz audio, against
    the routed group without input_rate fed the converted samples of the same pushes."""
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    S, PUSH = 2, 960
    emb, _ = tl.load_base_model("synthetic", max_batch=16)
    heads = [Head(max_batch=16, seed=s) for s in (1, 2, 3)]
    xs = [_speechlike(48000, 1.6, 21 + s) for s in range(S)]
    rs = Resampler(48000)
    ys = [rs.forward(x, centred=False) for x in xs]
    groups = [bsa.LiveRoutedGroup(emb, heads, S, max_routes=4, n_thresholds=2, fired_only=False, **kw) for kw in (dict(input_rate=48000), {})]
    assert groups[0].in_push_samples == PUSH and not hasattr(groups[1], "resampler")
    for g in groups:
        assert [g.attach(0, 0, "uno", (0.3, 0.6)), g.attach(1, 2, "tres", (0.2, 0.5)), g.attach(1, 1, "dos", (0.4, 0.7))] == [0, 1, 2]
    at, n_records = 0, 0
    for n in (7000, 960, 1, 20000, 33333, 15506):
        lo, hi = at // PUSH, (at + n) // PUSH
        chunks = {0: xs[0][at:at + n], 1: xs[1][at:at + n]} if lo % 2 == 0 else {1: xs[1][at:at + n], 0: xs[0][at:at + n]}
        got = groups[0].feed(chunks)
        want = groups[1].feed({s: ys[s][lo * HOP:hi * HOP] for s in range(S)})
        assert got == want and groups[0].last_records == groups[1].last_records
        n_records += sum(len(r) for r in got.values())
        at += n
        assert [groups[0].samples_seen(s) for s in range(S)] == [at] * S
    assert at == xs[0].size and n_records >= 1 and groups[0].windows_seen(0) == groups[1].windows_seen(0) == 31
    groups[0].reset(0)
    assert not bool(groups[0].rstates[0].any().cpu()) and bool(groups[0].rstates[1].any().cpu())
    for g in groups:
        g.close()
    rs.close()
