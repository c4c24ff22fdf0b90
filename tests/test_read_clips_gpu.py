"""input_data.read_clips / read_recording and the entry points that read files through them (convert=True, channel=...): bit-equal to
the existing readers where those apply (_read_wav, read_wav_at, decode_wav + to_sample_rate) and to the numpy restatement of the decode
(tests/util_pcm.py) fed through the same resampler everywhere else."""
import os

import numpy as np
import pytest

from multilingual_kws_amd import pcm, synth
from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding import input_data
from tests import util_pcm as up

pytestmark = pytest.mark.gpu
RATE, N = 16000, 16000

# (name, format, channels, rate, seconds): 0.4 s, exactly 1 s and 1.7 s at the model's rate and at others
CLIPS = [("a", "s16", 1, 16000, 0.4), ("b", "s16", 1, 16000, 1.0), ("c", "s16", 1, 16000, 1.7),
         ("d", "s16", 2, 48000, 0.4), ("e", "s16", 1, 48000, 1.0), ("f", "s16", 2, 48000, 1.7),
         ("g", "s16", 1, 44100, 1.0), ("h", "s24", 2, 48000, 1.7), ("i", "f32", 1, 44100, 0.4),
         ("j", "mulaw", 1, 8000, 1.7), ("k", "s24", 1, 16000, 1.0), ("l", "f32", 2, 16000, 0.4), ("m", "mulaw", 2, 8000, 0.4)]


def _write(path, fmt, channels, rate, pcm16, extensible=False):
    """pcm16 [frames, channels] int16 -> a WAV file in `fmt`."""
    with open(path, "wb") as fh:
        fh.write(up.wav_image(fmt, channels, rate, up.from_int16(fmt, pcm16), extensible=extensible))
    return str(path)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp("clips")
    out = {}
    for k, (name, fmt, channels, rate, seconds) in enumerate(CLIPS):
        frames = int(round(rate * seconds))
        x = synth.clips_int16(channels, frames, seed=0xC11B0000 + 16 * k).T          # the channels are different clips
        out[name] = _write(root / f"{name}.wav", fmt, channels, rate, x, extensible=(fmt == "s24"))
    return out


def _chain(path, channel, n=N):
    """The restatement fed through the chain: decoded in numpy, converted by to_sample_rate, padded or truncated as decode_wav does."""
    with open(path, "rb") as fh:
        image = fh.read()
    info = pcm.wav_info(image)
    x = up.decode_frames(info.format, info.channels, image[info.data_offset:info.data_offset + info.frames * info.frame_bytes], channel)
    if info.rate != RATE:
        x = input_data.to_sample_rate(x, info.rate, RATE) if x.shape[0] else x
    if n is None:
        return x
    return x[:n] if x.shape[0] >= n else np.concatenate([x, np.zeros(n - x.shape[0], np.float32)])


def _bits(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(np.uint32)


def test_read_clips_mixed_batch(clips):
    import torch
    names = [c[0] for c in CLIPS]
    got = input_data.read_clips([clips[n] for n in names])
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(names), N) and got.is_contiguous()
    for row, (name, fmt, channels, rate, seconds) in zip(_bits(got), CLIPS):
        if fmt == "s16" and rate == RATE:
            want = input_data._read_wav(clips[name], N)
        elif fmt == "s16":
            want = input_data.read_wav_at(clips[name], RATE, N)
        else:
            want = _chain(clips[name], 0)
        assert np.array_equal(row, want.view(np.uint32)), name
        assert np.array_equal(row, _chain(clips[name], 0).view(np.uint32)), name        # the restatement agrees with the readers
        if seconds < 1.0:
            assert row[int(RATE * seconds) + 1:].max() == 0 and row[:int(RATE * seconds)].any(), name
    # another length, the mix, file images instead of paths, and an order that puts the rates in other groups
    order = names[::-1]
    images = [open(clips[n], "rb").read() for n in order]
    got = input_data.read_clips(images, RATE, 27001, channel="mix")
    for row, name in zip(_bits(got), order):
        assert np.array_equal(row, _chain(clips[name], "mix", 27001).view(np.uint32)), name
    # a channel the stereo files have and the mono files lack
    stereo = [c[0] for c in CLIPS if c[2] == 2]
    got = input_data.read_clips([clips[n] for n in stereo], channel=1)
    for row, name in zip(_bits(got), stereo):
        assert np.array_equal(row, _chain(clips[name], 1).view(np.uint32)), name
        assert not np.array_equal(row, _chain(clips[name], 0).view(np.uint32)), name
    with pytest.raises(ValueError, match="channel 1 of file 1, which has 1 channels"):
        input_data.read_clips([clips["d"], clips["a"]], channel=1)
    assert tuple(input_data.read_clips([], RATE, 5).shape) == (0, 5)
    # one file, and a batch at one foreign rate only
    assert np.array_equal(_bits(input_data.read_clips([clips["h"]]))[0], _chain(clips["h"], 0).view(np.uint32))
    got = input_data.read_clips([clips["d"], clips["f"], clips["e"]], RATE, 40000)
    for row, name in zip(_bits(got), "dfe"):
        assert np.array_equal(row, input_data.read_wav_at(clips[name], RATE, 40000).view(np.uint32)), name


def test_read_recording(tmp_path):
    x = synth.clips_int16(2, 3 * 44100, seed=0x5EC0D000).T
    path = _write(tmp_path / "call.wav", "s16", 2, 44100, x)
    with open(path, "rb") as fh:
        first, rate = input_data.decode_wav(fh.read())
    want0 = input_data.to_sample_rate(first, rate, RATE)
    got = {ch: input_data.read_recording(path, RATE, ch) for ch in (0, 1, "mix")}
    assert got[0].is_cuda and tuple(got[0].shape) == (48000,) and np.array_equal(_bits(got[0]), want0.view(np.uint32))
    for ch in (1, "mix"):
        assert np.array_equal(_bits(got[ch]), _chain(path, ch, None).view(np.uint32))
        assert not np.array_equal(_bits(got[ch]), _bits(got[0]))
    # at the file's own rate nothing is converted: the samples themselves
    same = input_data.read_recording(path, 44100, 1)
    assert np.array_equal(_bits(same), (x[:, 1].astype(np.float32) / np.float32(32768)).view(np.uint32))
    # a 24-bit extensible copy, and an empty file
    p24 = _write(tmp_path / "call24.wav", "s24", 2, 44100, x, extensible=True)
    assert np.array_equal(_bits(input_data.read_recording(p24, RATE, "mix")), _chain(p24, "mix", None).view(np.uint32))
    empty = _write(tmp_path / "empty.wav", "s16", 2, 44100, x[:0])
    assert tuple(input_data.read_recording(empty).shape) == (0,)
    with pytest.raises(ValueError, match="channel 2 of a file with 2 channels"):
        input_data.read_recording(path, RATE, 2)


@pytest.fixture(scope="module")
def models():
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=128)
    return [tl.TransferLearnedModel(emb, Head(max_batch=128, seed=s), blob, "synthetic") for s in (1, 2, 3)]


@pytest.fixture(scope="module")
def copies(tmp_path_factory):
    """Ten canonical clips (16 kHz, 16-bit, mono, one second) and 48 kHz 24-bit stereo files of other clips."""
    root = tmp_path_factory.mktemp("copies")
    x = synth.clips_int16(10, 16000, seed=0xE7A10000)
    canon = [_write(root / f"c{i}.wav", "s16", 1, 16000, x[i][:, None]) for i in range(10)]
    wide = synth.clips_int16(20, 48000, seed=0xE7A20000)
    hi = [_write(root / f"w{i}.wav", "s24", 2, 48000, np.stack([wide[2 * i], wide[2 * i + 1]], axis=1), extensible=True) for i in range(10)]
    return canon, hi


def test_evaluate_files_many_convert(models, copies):
    import torch
    from multilingual_kws_amd.embedding import distance_filtering as df
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    canon, hi = copies
    ms = input_data.standard_microspeech_model_settings(3)
    plain = tl.evaluate_files_many(canon, models, ms)
    assert np.array_equal(tl.evaluate_files_many(canon, models, ms, convert=True).view(np.uint32), plain.view(np.uint32))
    got = tl.evaluate_files_many(hi, models, ms, as_device=True, convert=True)
    emb = models[0].embedding
    e = emb.forward(input_data.to_micro_spectrogram(ms, input_data.read_clips(hi, RATE, N)))
    for k, m in enumerate(models):
        assert torch.equal(got[k], m.head.forward(e)), k
    assert torch.equal(got, Head.forward_many([m.head for m in models], e))
    with pytest.raises(ValueError, match="only 16-bit PCM"):             # the default still takes what it took
        tl.evaluate_files_many(hi, models, ms)
    # the other bulk readers go through the same switch
    assert np.array_equal(df.embed_files(canon, emb, ms, convert=True), df.embed_files(canon, emb, ms))
    assert np.array_equal(df.embed_files(hi, emb, ms, convert=True), emb.predict(tl._specs_for_files(hi, ms, convert=True)))
    assert np.array_equal(tl._specs_for_files(hi, ms, convert=True), input_data.to_micro_spectrogram(ms, input_data.read_clips(hi)).cpu().numpy())
    curves = tl.classification_curves(models[:2], [hi[:5], hi[5:]], [hi[5:], hi[:5]], ms, convert=True)
    assert len(curves) == 2 and curves[0]["n_target"] == 5 and len(curves[0]["tprs"]) == len(curves[0]["fprs"])
    a = tl.classification_curves(models[:2], [canon[:5], canon[5:]], [canon[5:], canon[:5]], ms, convert=True)
    b = tl.classification_curves(models[:2], [canon[:5], canon[5:]], [canon[5:], canon[:5]], ms)
    assert all(np.array_equal(np.asarray(a[k][key]), np.asarray(b[k][key])) for k in range(2) for key in ("tprs", "fprs"))


def test_audio_dataset_convert(copies, tmp_path):
    canon, hi = copies
    bg = synth.clips_int16(2, 3 * 48000, seed=0xB6C00000).T // 8
    os.makedirs(tmp_path / "bg")
    bg_path = _write(tmp_path / "bg" / "noise.wav", "s24", 2, 48000, bg, extensible=True)
    ms = input_data.standard_microspeech_model_settings(3)
    ds = input_data.AudioDataset(ms, ["word"], str(tmp_path / "bg"), hi[5:], seed=1, convert=True)
    assert ds.background_sizes.tolist() == [48000]
    assert np.array_equal(ds.background_host[0].view(np.uint32), _bits(input_data.read_recording(bg_path, RATE)))
    assert np.array_equal(_bits(ds._upload_bank(hi[:5])), _bits(input_data.read_clips(hi[:5], RATE, N)))
    assert np.array_equal(_bits(ds._unknown()), _bits(input_data.read_clips(hi[5:], RATE, N)))
    # on canonical files the bank is the one the default uploads
    plain = input_data.AudioDataset(ms, ["word"], None, canon[5:], seed=1)
    assert np.array_equal(_bits(input_data.AudioDataset(ms, ["word"], None, canon[5:], seed=1, convert=True)._upload_bank(canon)),
                          _bits(plain._upload_bank(canon)))
    # and a training batch comes out of the converted banks
    spec, labels = next(iter(ds.init_single_target(input_data.AUTOTUNE, hi[:5], is_training=True).shuffle().repeat().batch(8)))
    assert tuple(spec.shape) == (8, 49, 40, 1) and tuple(labels.shape) == (8,) and bool(spec.isfinite().all())


def test_multi_keyword_detections_keeps_its_bits(models, tmp_path, capsys):
    import torch
    from multilingual_kws_amd import run
    keywords, thr = ["uno", "dos", "tres"], 0.34
    x = synth.clips_int16(2, 3 * 44100, seed=0xDE7EC000).T
    mono = _write(tmp_path / "mono.wav", "s16", 1, 44100, x[:, :1])
    stereo = _write(tmp_path / "stereo.wav", "s16", 2, 44100, x)
    ms = input_data.standard_microspeech_model_settings(3)
    with open(mono, "rb") as fh:
        first, rate = input_data.decode_wav(fh.read())
    converted = input_data.to_sample_rate(first, rate, RATE)                 # the explicit route of before
    seen, real = [], sa.streaming_inferences

    def spy(models_, ms_, audio, sample_rate, *a, **k):
        seen.append((audio, sample_rate))
        return real(models_, ms_, audio, sample_rate, *a, **k)
    sa.streaming_inferences = spy
    try:
        det = sa.multi_keyword_detections(keywords, models, mono, detection_threshold=thr, resample=True)
        audio, sr = seen.pop()
        assert sr == RATE and torch.is_tensor(audio) and np.array_equal(_bits(audio), converted.view(np.uint32))
        want = real(models, ms, converted, RATE, 1000, 20, max_chunk_length_sec=1200, as_device=True)
        flags = sa.StreamFlags(wav=mono, ground_truth=None, target_keyword="uno", detection_thresholds=[thr], max_chunk_length_sec=1200)
        found = sa.detect_many(want, flags, [thr], RATE, data_samples=converted.shape[0], keywords=keywords)
        merged = sorted([d for f in found for d in f[thr][1]], key=lambda d: d[1])
        assert det == dict(keywords=keywords, min_threshold=thr,
                           detections=[dict(keyword=d[0], time_ms=d[1], confidence=d[2], groundtruth="ng") for d in merged])
        # channel 0 of the stereo file is the mono file; channel 1 is heard through the same chain
        assert sa.multi_keyword_detections(keywords, models, stereo, detection_threshold=thr, resample=True) == det
        seen.clear()
        run.inference(keywords, models, stereo, detection_threshold=thr, resample=True, channel=1)
        audio, sr = seen.pop()
        assert sr == RATE and np.array_equal(_bits(audio), _chain(stereo, 1, None).view(np.uint32))
        with pytest.raises(ValueError, match="needs resample=True"):
            sa.multi_keyword_detections(keywords, models, stereo, detection_threshold=thr, channel="mix")
    finally:
        sa.streaming_inferences = real
    capsys.readouterr()
