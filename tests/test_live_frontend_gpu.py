"""mkws_frontend_live_push_f32: the streaming frontend fed push by push with its state on the device, held bit for bit to
mkws_frontend_stream_f32 over the whole recording (Frontend.stream) and, for three windows, to the C oracle."""
import numpy as np
import pytest

from multilingual_kws_amd.frontend import Frontend, live_window_time_ms, live_windows
from oracle.frontend_oracle import FrontendOracle
from tests.util_data import tone_clip

pytestmark = pytest.mark.gpu
CLIP, HOP, SAMPLES = 16000, 320, 25600
CONFIGS = [{}, dict(window_size_ms=25, window_step_ms=10, num_channels=32)]     # the second one's carried tail spans more than two steps


def _recording():
    rng = np.random.default_rng(5)
    pcm = np.concatenate([tone_clip(f, rng, n=6400, amp=a) for f, a in ((440, 9000), (1900, 3000), (700, 12000), (3100, 6000))])
    return pcm.astype(np.float32) / 32768


def _push_all(fe, d_audio, h, state, first_push=0, snapshot_after=None):
    """Pushes first_push .. of the recording, no synchronisation in between -> (spec [P, h, F, C], raw, meta [P, 2 + h], snapshot)."""
    import torch
    P = SAMPLES // (h * HOP)
    F = fe.stream(d_audio[:CLIP], CLIP, HOP).shape[1]
    spec = torch.full((P, h, F, fe.num_channels), -1.0, dtype=torch.float32, device="cuda")
    raw = torch.full((P, h, F, fe.num_channels), -1, dtype=torch.int16, device="cuda")
    meta = torch.full((P, 2 + h), -1, dtype=torch.int64, device="cuda")
    snap = None
    for i in range(first_push, P):
        fe.live_push(state, d_audio[i * h * HOP:(i + 1) * h * HOP], CLIP, HOP, h, spec=spec[i], raw=raw[i], meta=meta[i])
        if snapshot_after is not None and i + 1 == snapshot_after:
            snap = state.clone()
    return spec.cpu().numpy(), raw.cpu().numpy(), meta.cpu().numpy(), snap


@pytest.mark.parametrize("h", [1, 4])
@pytest.mark.parametrize("over", CONFIGS)
def test_live_pushes_equal_the_stream_form(over, h):
    import torch
    audio = _recording()
    d_audio = torch.from_numpy(audio).cuda()
    fe = Frontend(max_samples=SAMPLES, **over)
    want_spec, want_raw = (x.cpu().numpy() for x in fe.stream(d_audio, CLIP, HOP, want_raw=True))
    W = live_windows(SAMPLES, CLIP, HOP)
    assert W == 31 == want_spec.shape[0]
    state = fe.live_state(CLIP, HOP, h)
    spec, raw, meta, snap = _push_all(fe, d_audio, h, state, snapshot_after=40 if h == 1 else None)
    assert int(state[0].cpu()) == SAMPLES                                  # the position is the block's first int64
    seen, emitted = 0, 0
    for i in range(meta.shape[0]):
        first, after = live_windows(seen, CLIP, HOP), live_windows(seen + h * HOP, CLIP, HOP)
        count = after - first
        assert meta[i, 0] == count and meta[i, 1] == first, i
        if seen + h * HOP < CLIP:
            assert count == 0                                              # the first second fills: nothing to emit
        assert meta[i, 2:2 + count].tolist() == [live_window_time_ms(w, HOP) for w in range(first, after)] and (meta[i, 2 + count:] == -1).all()
        assert np.array_equal(raw[i, :count], want_raw[first:after]) and np.array_equal(spec[i, :count], want_spec[first:after]), i
        assert (raw[i, count:] == -1).all() and (spec[i, count:] == -1).all()     # rows past count are left untouched
        seen, emitted = seen + h * HOP, emitted + count
    assert emitted == W
    # three windows against the C oracle
    fo = FrontendOracle(**over)
    for w in (0, 13, 30):
        ref_spec, ref_raw = fo.run_batch_f32(audio[None, w * HOP:w * HOP + CLIP], want_u16=True)
        assert np.array_equal(want_raw[w].view(np.uint16), ref_raw[0]) and np.array_equal(want_spec[w], ref_spec[0])
    if h == 1:
        # the snapshot taken after push 40, restored after push 80 (and after 60 more below), continues from push 41
        state.copy_(snap)
        assert int(state[0].cpu()) == 40 * HOP
        spec2, raw2, meta2, _ = _push_all(fe, d_audio, 1, state, first_push=40)
        assert np.array_equal(raw2[40:], raw[40:]) and np.array_equal(spec2[40:], spec[40:]) and np.array_equal(meta2[40:], meta[40:])
        assert meta[40:, 0].sum() > 0
    fe.close()


def test_snapshot_taken_after_push_40_restored_after_push_60():
    import torch
    d_audio = torch.from_numpy(_recording()).cuda()
    fe = Frontend(max_samples=SAMPLES)
    state = fe.live_state(CLIP, HOP, 1)
    outs = []
    for i in range(60):
        outs.append(fe.live_push(state, d_audio[i * HOP:(i + 1) * HOP], CLIP, HOP, 1, want_raw=True))
        if i + 1 == 40:
            snap = state.clone()
    state.copy_(snap)
    for i in range(40, 60):
        spec, raw, meta = fe.live_push(state, d_audio[i * HOP:(i + 1) * HOP], CLIP, HOP, 1, want_raw=True)
        assert torch.equal(spec, outs[i][0]) and torch.equal(raw, outs[i][1]) and torch.equal(meta, outs[i][2]), i
    assert meta.tolist() == [1, 10, 200]
    # a zeroed block is a fresh stream
    state.zero_()
    spec, none, meta = fe.live_push(state, d_audio[:HOP], CLIP, HOP, 1)
    assert none is None
    assert meta[:2].tolist() == [0, 0] and int(state[0].cpu()) == HOP
    with pytest.raises(ValueError, match="frame step"):
        fe.live_state(CLIP, 300, 1)                                        # not a multiple of the frame step
    assert fe.L.mkws_frontend_live_push_f32(fe.h, state.data_ptr(), d_audio.data_ptr(), CLIP, 300, 1, spec.data_ptr(), None, meta.data_ptr(), None) == -2
    assert fe.L.mkws_frontend_live_push_f32(fe.h, None, d_audio.data_ptr(), CLIP, HOP, 1, spec.data_ptr(), None, meta.data_ptr(), None) == -1
    assert fe.L.mkws_frontend_live_push_f32(fe.h, state.data_ptr(), d_audio.data_ptr(), CLIP, HOP, 0, spec.data_ptr(), None, meta.data_ptr(), None) == -1
    torch.cuda.synchronize()
    fe.close()


def test_a_push_of_more_hops_than_a_workgroup_has_threads():
    """300 hops per push: d_meta's times are written by a 256-thread workgroup, one push completes up to 300 windows."""
    import torch
    h, n = 300, 2 * 300 * HOP
    rng = np.random.default_rng(6)
    audio = np.concatenate([tone_clip(300 + 170 * k, rng, n=16000) for k in range(12)]).astype(np.float32) / 32768
    d_audio = torch.from_numpy(audio).cuda()
    fe = Frontend(max_samples=n)
    want_spec, want_raw = fe.stream(d_audio, CLIP, HOP, want_raw=True)
    W = live_windows(n, CLIP, HOP)
    assert W == 551 == want_spec.shape[0]
    state = fe.live_state(CLIP, HOP, h)
    seen = 0
    for i in range(2):
        meta = torch.full((2 + h,), -1, dtype=torch.int64, device="cuda")
        spec, raw, meta = fe.live_push(state, d_audio[i * h * HOP:(i + 1) * h * HOP], CLIP, HOP, h, meta=meta, want_raw=True)
        first, after = live_windows(seen, CLIP, HOP), live_windows(seen + h * HOP, CLIP, HOP)
        count = after - first
        assert count == (251, 300)[i]
        assert meta.tolist() == [count, first] + [live_window_time_ms(w, HOP) for w in range(first, after)] + [-1] * (h - count)
        assert torch.equal(raw[:count], want_raw[first:after]) and torch.equal(spec[:count], want_spec[first:after])
        seen += h * HOP
    assert int(state[0].cpu()) == n
    fe.close()

