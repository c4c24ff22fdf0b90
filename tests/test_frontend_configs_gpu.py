"""-m gpu: the frontend kernels against the C oracle, bit for bit, on the configuration matrix of tests/util_frontend_cases.py -- every
clip of every configuration compared in full, no tolerance.  tests/test_frontend_cases_cpu.py states which branch of
mkws_frontend.hip each configuration is there for."""
import numpy as np
import pytest

from multilingual_kws_amd.frontend import Frontend, live_window_time_ms, live_windows, num_frames
from oracle.frontend_oracle import FrontendOracle
from tests.util_frontend_cases import CASES, case_expected, case_signals, full_cfg, stream_geometry, stream_recording

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SCALE = np.float32(10.0 / 256.0)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _check(fe, audio, exp, log_on, what):
    """forward(audio) == the oracle's raw integers (and the scaled features where log is on) -> the device outputs."""
    spec, raw = fe.forward(audio, want_raw=True)
    got = _u16(raw)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} of {exp.size} values differ, first at (clip, frame, channel) {bad[0].tolist()}"
    if log_on:
        assert np.array_equal(spec.cpu().numpy(), exp.astype(np.float32) * SCALE), what
    return spec, raw


@pytest.mark.parametrize("name", list(CASES))
def test_forward_every_configuration(name):
    over, n = CASES[name]
    log_on = bool(full_cfg(name)["enable_log"])
    pcm, exp = case_signals(name), case_expected(name)
    assert len(np.unique(exp)) > 100                                       # the reference is not degenerate
    fe = Frontend(max_samples=n, **over)
    d_i16 = torch.from_numpy(pcm.copy()).cuda()
    d_f32 = torch.from_numpy(pcm.astype(np.float32) / 32768).cuda()
    spec_i, raw_i = _check(fe, d_i16, exp, log_on, f"{name} int16")
    spec_f, raw_f = _check(fe, d_f32, exp, log_on, f"{name} float32")
    assert torch.equal(raw_i, raw_f) and torch.equal(spec_i, spec_f)
    for d in (d_i16, d_f32):                                               # batch-size invariant, deterministic
        one_spec, one_raw = fe.forward(d[3:4].clone(), want_raw=True)
        assert torch.equal(one_raw[0], raw_i[3]) and torch.equal(one_spec[0], spec_i[3])
        again_spec, again_raw = fe.forward(d, want_raw=True)
        assert torch.equal(again_raw, raw_i) and torch.equal(again_spec, spec_i)
    fe.close()


@pytest.mark.parametrize("name", ["default", "sr22050_nolog", "sr11025"])
def test_unaligned_inputs(name):
    """Loads off the pair boundary: clips one sample shorter (rows at odd offsets, int16 too) and a base pointer one element past a
    pair boundary, which forward must take as it is."""
    over, n = CASES[name]
    log_on = bool(full_cfg(name)["enable_log"])
    pcm = case_signals(name)
    B = pcm.shape[0]
    fe = Frontend(max_samples=n, **over)
    for dtype, mod, rem in ((torch.int16, 4, 2), (torch.float32, 8, 4)):
        host = torch.from_numpy(pcm.copy()) if dtype == torch.int16 else torch.from_numpy(pcm.astype(np.float32) / 32768)
        short = host[:, :n - 1].contiguous().cuda()
        _check(fe, short, case_expected(name, None, 1), log_on, f"{name} {dtype} n - 1")
        flat = torch.zeros(B * n + 8, dtype=dtype, device="cuda")
        assert flat.data_ptr() % 8 == 0
        audio = flat[1:1 + B * n].view(B, n)
        audio.copy_(host)
        assert audio.data_ptr() % mod == rem and audio.is_contiguous() and audio.contiguous().data_ptr() == audio.data_ptr()
        _check(fe, audio, case_expected(name), log_on, f"{name} {dtype} base pointer off the pair boundary")
    fe.close()


def _live_run(fe, d_audio, window, hop, h, n_pushes, states=None):
    """n_pushes pushes of h hops, no synchronisation in between.  d_audio [n] with a one-stream state, or [S, n] with the states of
    live_state_many -> (spec [P, S * h, F, C], raw, meta [P, S, 2 + h], state), outputs prefilled with -1."""
    many = states is not None
    S = states.shape[0] if many else 1
    state = states if many else fe.live_state(window, hop, h)
    F = num_frames(fe.cfg, window)
    spec = torch.full((n_pushes, S * h, F, fe.num_channels), -1.0, dtype=torch.float32, device="cuda")
    raw = torch.full((n_pushes, S * h, F, fe.num_channels), -1, dtype=torch.int16, device="cuda")
    meta = torch.full((n_pushes, S, 2 + h), -1, dtype=torch.int64, device="cuda")
    for i in range(n_pushes):
        if many:
            fe.live_push_many(state, d_audio[:, i * h * hop:(i + 1) * h * hop].contiguous(), window, hop, h, spec=spec[i], raw=raw[i], meta=meta[i])
        else:
            fe.live_push(state, d_audio[i * h * hop:(i + 1) * h * hop], window, hop, h, spec=spec[i], raw=raw[i], meta=meta[i, 0])
    return spec.cpu().numpy(), raw.cpu().numpy().view(np.uint16), meta.cpu().numpy(), state


@pytest.mark.parametrize("name", ["c64_nopcan", "sr22050_nolog", "sr11025", "w512", "w272"])
def test_stream_and_live_forms(name):
    """Frontend.stream == the oracle on every window's slice; live pushes of 1 and 3 hops concatenate to the stream result with the meta
    contract of test_live_pushes_equal_the_stream_form; three streams in lockstep == three one-stream runs."""
    over = CASES[name][0]
    cfg = full_cfg(name)
    window, hop, total = stream_geometry(name)
    rec = stream_recording(name)
    rolls = (0, 7, 1 + cfg["window_size_ms"] * cfg["sample_rate"] // 1000)
    # the pushes are whole: the live forms are fed the recording plus the zeros that fill its last push of three hops
    fed = -(-total // (3 * hop)) * 3 * hop
    recs = np.stack([np.concatenate([np.roll(rec, r), np.zeros(fed - total, np.int16)]) for r in rolls])
    fo = FrontendOracle(**over)
    fe = Frontend(max_samples=fed, **over)
    d_recs = torch.from_numpy(recs.astype(np.float32) / 32768).cuda()
    W, Wp = live_windows(total, window, hop), live_windows(fed, window, hop)
    assert W == 41 and W <= Wp <= W + 2
    want_raw, want_spec = [], []
    for s in range(3):
        exp = np.stack([fo.run_i16(recs[s, w * hop:w * hop + window]) for w in range(Wp)])
        assert exp.shape == (Wp, 21, cfg["num_channels"]) and len(np.unique(exp)) > 50
        for n, nw in ((total, W), (fed, Wp)):
            sp, raw = fe.stream(d_recs[s, :n], window, hop, want_raw=True)
            bad = np.argwhere(_u16(raw) != exp[:nw])
            assert bad.shape[0] == 0, f"{name} stream {s}: {bad.shape[0]} values differ, first at (window, frame, channel) {bad[0].tolist()}"
            if cfg["enable_log"]:
                assert np.array_equal(sp.cpu().numpy(), exp[:nw].astype(np.float32) * SCALE)
        want_raw.append(exp)
        want_spec.append(sp.cpu().numpy())
    for h in (1, 3):
        P = fed // (h * hop)
        ones = [_live_run(fe, d_recs[s], window, hop, h, P) for s in range(3)]
        for s, (spec, raw, meta, state) in enumerate(ones):
            assert int(state[0].cpu()) == fed
            seen, rows_raw, rows_spec = 0, [], []
            for i in range(P):
                first, after = live_windows(seen, window, hop), live_windows(seen + h * hop, window, hop)
                count = after - first
                assert meta[i, 0, 0] == count and meta[i, 0, 1] == first, (s, i)
                assert meta[i, 0, 2:2 + count].tolist() == [live_window_time_ms(w, hop, cfg["sample_rate"]) for w in range(first, after)]
                assert (meta[i, 0, 2 + count:] == -1).all()
                assert (raw[i, count:] == 0xFFFF).all() and (spec[i, count:] == -1).all()       # rows past count are left untouched
                rows_raw.append(raw[i, :count])
                rows_spec.append(spec[i, :count])
                seen += h * hop
            got = np.concatenate(rows_raw)
            assert got.shape[0] == Wp
            bad = np.argwhere(got != want_raw[s])
            assert bad.shape[0] == 0, f"{name} live h={h} stream {s}: {bad.shape[0]} values differ, first at (window, frame, channel) {bad[0].tolist()}"
            assert np.array_equal(np.concatenate(rows_spec), want_spec[s])
        m_spec, m_raw, m_meta, m_state = _live_run(fe, d_recs, window, hop, h, P, states=fe.live_state_many(3, window, hop, h))
        for s, (spec, raw, meta, state) in enumerate(ones):
            assert np.array_equal(m_meta[:, s], meta[:, 0]), (h, s)
            assert np.array_equal(m_raw[:, s * h:(s + 1) * h], raw) and np.array_equal(m_spec[:, s * h:(s + 1) * h], spec), (h, s)
            assert torch.equal(m_state[s], state), (h, s)
    fe.close()
