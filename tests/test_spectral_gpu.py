"""-m gpu: the mfcc / average kernels (mkws_spectral.hip) against the float64 reference of tests/spectral_cases.py at the tolerances its
float32 twin measured (T_POWER, T_MEL: abs err / frame max; T_FEAT: abs err; tests/test_spectral_cpu.py pins how they were measured), and
the contracts of include/mkws.h, each exact."""
import ctypes

import numpy as np
import pytest

import util_fenced as uf
from multilingual_kws_amd import _lib, spectral, synth
from multilingual_kws_amd.embedding import batch_streaming_analysis, input_data
from tests import spectral_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _host(t):
    return t.cpu().numpy()


def _forward_all(fe, audio):
    """-> dict(power=, mel= (mfcc), feat=) of device tensors"""
    if fe.cfg.mode == spectral.MFCC:
        feat, power, mel = fe.forward(audio, want_power=True, want_mel=True)
        return dict(feat=feat, power=power, mel=mel)
    feat, power = fe.forward(audio, want_power=True)
    return dict(feat=feat, power=power)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_every_configuration_against_float64(geometry, mode):
    """Every geometry x mode on the eight inputs: power and mel taps on all of them, the features on the inputs with a noise floor and on
    silence; taps off, a second call and a one-clip call give the same bits."""
    cfg = sc.cfg_of(geometry, mode)
    audio_np = sc.input_batch(geometry)
    want = sc.reference_of(geometry, mode)
    fe = spectral.SpectralFrontend(max_samples=16000, **cfg)
    audio = torch.from_numpy(audio_np).cuda()
    got = _forward_all(fe, audio)
    host = {k: _host(v) for k, v in got.items()}
    assert all(host[k].shape == want[k].shape for k in want), {k: host[k].shape for k in host}
    e_power, e_mel, e_feat = sc.layer_errors(cfg, host, want)
    print(f"{geometry} {mode}: power {e_power:.3e} (T {sc.T_POWER}), mel {e_mel:.3e} (T {sc.T_MEL}), features {e_feat:.3e} (T {sc.T_FEAT})")
    assert np.isfinite(host["feat"]).all()
    assert e_power <= sc.T_POWER and e_mel <= sc.T_MEL and e_feat <= sc.T_FEAT, (e_power, e_mel, e_feat)
    if cfg["mode"] == "mfcc":
        s = host["feat"][sc.INPUTS.index("silence")]
        assert np.abs(s[:, 0] - np.sqrt(2 / 40) * 40 * np.log(1e-12)).max() <= sc.T_FEAT and (s.shape[1] == 1 or np.abs(s[:, 1:]).max() <= sc.T_FEAT)
    else:
        assert not host["feat"][sc.INPUTS.index("silence")].any()
    plain = fe.forward(audio)                                               # taps NULL
    assert torch.equal(plain, got["feat"])
    again = _forward_all(fe, audio)                                         # deterministic
    assert all(torch.equal(again[k], got[k]) for k in got)
    one = _forward_all(fe, audio[4:5].clone())                              # a clip does not depend on its batch
    assert all(torch.equal(one[k][0], got[k][4]) for k in got)
    fe.close()


@pytest.mark.parametrize("B", sc.BATCHES)
@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_shapes(geometry, B):
    """B in {1, 3, 65} x n in {no frames, one frame, tail ignored, the standard clip, odd rows}: features and power against float64; at the
    odd row length every row equals the one-clip call on it (rows 1.. are not 16-byte aligned, row 0 is), bit for bit."""
    for mode in ("mfcc40", "avg6"):
        cfg = sc.cfg_of(geometry, mode)
        fe = spectral.SpectralFrontend(max_samples=16001, **cfg)
        for n in sc.shape_samples(geometry):
            audio_np = synth.clips_float32(B, n)
            want = sc.reference(cfg, audio_np)
            audio = torch.from_numpy(audio_np).cuda()
            got = _forward_all(fe, audio)
            host = {k: _host(v) for k, v in got.items()}
            F = spectral.num_frames(fe.cfg, n)
            assert host["feat"].shape == want["feat"].shape == (B, F, fe.width) and host["power"].shape == (B, F, fe.bins), (n, host["feat"].shape)
            if F == 0:
                continue
            e_power = sc.frame_rel_err(host["power"], want["power"])
            if mode == "mfcc40":
                e_feat, tol = sc.abs_err(host["feat"], want["feat"]), sc.T_FEAT
                assert sc.frame_rel_err(host["mel"], want["mel"]) <= sc.T_MEL
            else:
                top = np.max(want["power"], axis=-1, keepdims=True)
                e_feat, tol = float(np.max(np.abs(host["feat"] - want["feat"]) / top)), sc.T_POWER
            print(f"{geometry} {mode} B={B} n={n}: power {e_power:.3e}, features {e_feat:.3e} (T {tol})")
            assert e_power <= sc.T_POWER and e_feat <= tol, (mode, n, e_power, e_feat)
            if n == 16001:
                for b in sorted({0, min(1, B - 1), B // 2, B - 1}):
                    one = _forward_all(fe, audio[b:b + 1].clone())
                    assert all(torch.equal(one[k][0], got[k][b]) for k in got), (mode, b)
        fe.close()


@pytest.mark.parametrize("geometry", list(sc.GEOMETRIES))
def test_int16_input_is_float32_input_of_pcm_over_32768(geometry):
    for mode, n in (("mfcc40", 16001), ("avg6", 16000)):
        fe = spectral.SpectralFrontend(max_samples=n, **sc.cfg_of(geometry, mode))
        pcm = synth.clips_int16(3, n)
        pcm[0, :4] = [-32768, 32767, 0, -1]
        a = _forward_all(fe, torch.from_numpy(pcm).cuda())
        b = _forward_all(fe, torch.from_numpy(pcm.astype(np.float32) / np.float32(32768)).cuda())
        assert all(torch.equal(a[k], b[k]) for k in a), (mode, n)
        assert bool(a["feat"].isfinite().all()) and float(a["power"].max()) > 0
        fe.close()


@pytest.mark.parametrize("mode", ["mfcc40", "mfcc13", "avg6"])
def test_out_inside_a_canary_arena(mode):
    """forward(out=) into the middle of [pad | B * frames * width | pad] of NaN canaries: pads intact, every element written, the same bits
    as the call that allocates; then the C call with every buffer fenced, the taps too, and the audio between canaries."""
    cfg = sc.cfg_of("w480", mode)
    fe = spectral.SpectralFrontend(max_samples=16001, **cfg)
    B, n = 3, 16001
    audio_np = synth.clips_float32(B, n)
    audio = torch.from_numpy(audio_np).cuda()
    want = _forward_all(fe, audio)
    F, W = 49, fe.width
    fb = uf.FencedBuffer(B * F * W)
    got = fe.forward(audio, out=fb.mid.view(B, F, W))
    torch.cuda.synchronize()
    assert fb.pads_intact() and not fb.canary_mask().any() and torch.equal(got, want["feat"])
    mfcc = cfg["mode"] == "mfcc"
    f_audio = uf.FencedBuffer(B * n, fill=audio_np)
    f_feat, f_power, f_mel = uf.FencedBuffer(B * F * W), uf.FencedBuffer(B * F * fe.bins), uf.FencedBuffer(B * F * 40)
    rc = fe.L.mkws_spectral_forward_f32(fe.h, f_audio.ptr(), B, n, f_feat.ptr(), f_power.ptr(), f_mel.ptr() if mfcc else None, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert all(f.pads_intact() for f in (f_audio, f_feat, f_power, f_mel))
    assert torch.equal(f_feat.mid.view(B, F, W), want["feat"]) and torch.equal(f_power.mid.view(B, F, fe.bins), want["power"])
    assert torch.equal(f_mel.mid.view(B, F, 40), want["mel"]) if mfcc else bool(f_mel.canary_mask().all())
    if not mfcc:                                                            # the average mode has no filterbank to tap: refused, nothing written
        f_feat.reset()
        assert fe.L.mkws_spectral_forward_f32(fe.h, f_audio.ptr(), B, n, f_feat.ptr(), None, f_mel.ptr(), _lib.current_stream_ptr()) == -1
        torch.cuda.synchronize()
        assert bool(f_feat.canary_mask().all()) and bool(f_mel.canary_mask().all())
    fe.close()


def test_refusals_of_the_device_calls():
    fe = spectral.SpectralFrontend(max_samples=16000)
    audio = torch.zeros((2, 16000), device="cuda")
    with pytest.raises(ValueError, match="max_samples"):
        fe.forward(torch.zeros((1, 16001), device="cuda"))
    with pytest.raises(ValueError, match="CUDA"):
        fe.forward(torch.zeros((1, 16000)))
    with pytest.raises(ValueError, match="out"):
        fe.forward(audio, out=torch.empty((1, 49, 40), device="cuda"))
    L, s = fe.L, _lib.current_stream_ptr()
    out = torch.empty((2, 49, 40), device="cuda")
    assert L.mkws_spectral_forward_f32(fe.h, audio.data_ptr(), 2, 16001, out.data_ptr(), None, None, s) == -1
    assert L.mkws_spectral_forward_f32(fe.h, audio.data_ptr(), -1, 16000, out.data_ptr(), None, None, s) == -1
    assert L.mkws_spectral_forward_f32(fe.h, None, 2, 16000, out.data_ptr(), None, None, s) == -1
    assert L.mkws_spectral_forward_f32(fe.h, audio.data_ptr(), 2, 16000, None, None, None, s) == -1
    assert L.mkws_spectral_forward_f32(fe.h, None, 0, 16000, None, None, None, s) == 0            # nothing to do, nothing launched
    assert L.mkws_spectral_forward_f32(fe.h, None, 2, 479, None, None, None, s) == 0
    assert L.mkws_spectral_stream_f32(fe.h, audio.data_ptr(), 16000, 16000, 321, out.data_ptr(), 1, s) == -2
    assert b"hop_samples" in L.mkws_last_error()
    assert L.mkws_spectral_stream_f32(fe.h, audio.data_ptr(), 16000, 8000, 320, out.data_ptr(), 1, s) == -1     # 26 windows, room for one
    assert L.mkws_spectral_stream_f32(fe.h, None, 15999, 16000, 320, None, 0, s) == 0
    fe.close()


@pytest.mark.parametrize("geometry,mode", [("w480", "mfcc40"), ("w400", "mfcc13"), ("w640", "avg6"), ("w129", "mfcc40")])
def test_stream_equals_forward_on_the_cut_windows(geometry, mode):
    """3 s of audio, hop = stride and hop = 2 * stride: row w of stream() is forward() on samples [w * hop, w * hop + window), bit for bit."""
    sr, window, stride = sc.GEOMETRIES[geometry]
    n, clip = 3 * sr, sr
    fe = spectral.SpectralFrontend(max_samples=n, **sc.cfg_of(geometry, mode))
    rec = torch.from_numpy(np.concatenate([synth.clips_float32(2, sr).reshape(-1), sc.signals(sr, sr)["chirp"]])).cuda()
    assert rec.shape == (n,)
    for hop in (stride, 2 * stride):
        got = fe.stream(rec, clip, hop)
        nw = 1 + (n - clip) // hop
        assert tuple(got.shape) == (nw, spectral.num_frames(fe.cfg, clip), fe.width)
        idx = torch.arange(clip, device="cuda")[None] + hop * torch.arange(nw, device="cuda")[:, None]
        for lo in range(0, nw, 64):                       # (the cut windows in batches: the forward form is one workgroup per window)
            assert torch.equal(got[lo:lo + 64], fe.forward(rec[idx[lo:lo + 64]])), (hop, lo)
    short = fe.stream(rec[:clip - 1], clip, stride)       # shorter than a window: 0 windows, nothing launched
    assert tuple(short.shape) == (0, spectral.num_frames(fe.cfg, clip), fe.width)
    with pytest.raises(ValueError, match="hop_samples"):
        fe.stream(rec, clip, stride + 1)
    fe.close()


@pytest.mark.parametrize("mode", ["mfcc40", "avg6"])
def test_forward_is_capturable(mode):
    """A forward recorded in a torch.cuda.graph and replayed on new input gives the eager call's bits."""
    fe = spectral.SpectralFrontend(max_samples=16000, **sc.cfg_of("w480", mode))
    first, second = (torch.from_numpy(synth.clips_float32(5, 16000, first_clip=k)).cuda() for k in (0, 5))
    want = [fe.forward(a) for a in (first, second)]
    assert not torch.equal(want[0], want[1])
    static_in, static_out = first.clone(), torch.empty_like(want[0])
    chain = lambda: fe.forward(static_in, out=static_out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for a, w in ((second, want[1]), (first, want[0])):
        static_in.copy_(a)
        static_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, w)
    fe.close()


@pytest.fixture(scope="module")
def fewshot(tmp_path_factory):
    return synth.write_fewshot_dataset(str(tmp_path_factory.mktemp("spectral_fewshot")), n_unknown=16, n_bg=2, bg_seconds=4)


def test_audio_dataset_with_mfcc_settings(fewshot):
    ms = input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, "mfcc")
    ds = input_data.AudioDataset(ms, ["target"], fewshot["bg_dir"], fewshot["unknown"], unknown_percentage=50.0,
                                 spec_aug_params=input_data.SpecAugParams(percentage=0), seed=3)
    spec, labels = next(iter(ds.init_single_target(input_data.AUTOTUNE, fewshot["train"], is_training=True).shuffle(100).repeat().batch(12)))
    assert tuple(spec.shape) == (12, 49, 40, 1) and spec.dtype == torch.float32 and tuple(labels.shape) == (12,)
    want = sc.reference(sc.cfg_of("w480", "mfcc40"), _host(ds.last_audio))["feat"]
    err = sc.abs_err(_host(spec)[..., 0], want)
    print(f"AudioDataset mfcc batch against float64 of its own last_audio: {err:.3e} (T {sc.T_FEAT})")
    assert err <= sc.T_FEAT
    assert float(spec.min()) >= input_data.get_features_range(ms)[0] - 1.0           # nothing lies below digital silence


def test_file2spec_and_to_features(fewshot):
    ms = input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, "mfcc")
    got = input_data.file2spec(ms, fewshot["train"][0])
    assert isinstance(got, np.ndarray) and got.shape == (49, 40) and got.dtype == np.float32
    audio = input_data._read_wav(fewshot["train"][0], 16000)
    assert sc.abs_err(got, sc.reference(sc.cfg_of("w480", "mfcc40"), np.asarray(audio)[None])["feat"][0]) <= sc.T_FEAT
    batch = torch.from_numpy(synth.clips_float32(3, 16000)).cuda()
    dev = input_data.to_features(ms, batch)
    assert dev.is_cuda and tuple(dev.shape) == (3, 49, 40) and torch.equal(input_data.to_features(ms, batch[1]), dev[1])
    avg = input_data.prepare_model_settings(3, 16000, 1000, 30, 20, 40, "average")
    a = input_data.to_features(avg, synth.clips_float32(2, 16000))
    assert isinstance(a, np.ndarray) and a.shape == (2, 49, 43)
    want = sc.reference(sc.cfg_of("w480", "avg6"), synth.clips_float32(2, 16000))
    assert float(np.max(np.abs(a - want["feat"]) / want["power"].max(axis=-1, keepdims=True))) <= sc.T_POWER
    # stream_spectrograms dispatches the same way
    rec = np.concatenate([synth.clips_float32(2, 16000).reshape(-1)])
    sp = batch_streaming_analysis.stream_spectrograms(ms, rec, 16000, 320)
    assert len(batch_streaming_analysis.window_offsets(32000, 16000, 320)) == 50            # range(0, n - clip, stride): the last window is left out
    assert tuple(sp.shape) == (50, 49, 40) and torch.equal(sp[49], input_data.to_features(ms, torch.from_numpy(rec[49 * 320:49 * 320 + 16000]).cuda()))
