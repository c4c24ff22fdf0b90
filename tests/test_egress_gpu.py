"""The writers built on mkws_pcm_encode (input_data.encode_wav / write_clips / convert_clips, word_extraction.extract_shots,
batch_streaming_analysis.extract_detections) on the device: round trips through the readers, and the files' bytes against numpy slicing
plus the tests' restatement of the encode rule (tests/util_pcm_encode.py)."""
import os

import numpy as np
import pytest

from multilingual_kws_amd import pcm
from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding import input_data, word_extraction
from tests import util_pcm as up
from tests import util_pcm_encode as ue

pytestmark = pytest.mark.gpu
GRID = {"s16": 32768, "s24": 8388608, "u8": 128}
LENGTHS = [16000, 15999, 7]


def _on_grid(fmt, shape, seed):
    """float32 audio that lies on format fmt's own grid (k / scale, every k of the format), so that encoding loses nothing."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return rng.uniform(-1.5, 1.5, shape).astype(np.float32)
    scale = GRID[fmt]
    return rng.integers(-scale, scale, shape).astype(np.float32) / np.float32(scale)


def _body(image):
    info = pcm.wav_info(image)
    return info, bytes(image[info.data_offset:info.data_offset + info.frames * info.frame_bytes])


@pytest.mark.parametrize("fmt", ["s16", "s24", "u8", "f32"])
def test_read_clips_inverts_encode_wav(fmt):
    import torch
    x = _on_grid(fmt, (3, 16000), 1)
    images = input_data.encode_wav(torch.from_numpy(x).cuda(), 16000, fmt, lengths=LENGTHS)
    want = x.copy()
    for row, n in enumerate(LENGTHS):
        want[row, n:] = 0
        info, body = _body(images[row])
        assert (info.format, info.channels, info.rate, info.frames) == (fmt, 1, 16000, n)
        assert len(images[row]) == info.data_offset + len(body) + (len(body) & 1)
        assert body == ue.encode(fmt, x[row, :n]).tobytes()
    back = input_data.read_clips(images, 16000, 16000)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the host path writes the same files
    assert input_data.encode_wav(x, 16000, fmt, lengths=LENGTHS) == images


@pytest.mark.parametrize("fmt", ["mulaw", "alaw", "s32", "f64"])
def test_encode_wav_fades_and_gain(fmt):
    """The other formats, with a fade and a gain, against the restatement; a 1-D tensor is one file."""
    import torch
    x = np.random.default_rng(2).uniform(-1.2, 1.2, 4001).astype(np.float32)
    image, = input_data.encode_wav(torch.from_numpy(x).cuda(), 8000, fmt, fade_ms=25, gain=0.7)
    info, body = _body(image)
    assert (info.format, info.rate, info.frames) == (fmt, 8000, 4001)
    assert body == ue.item_bytes(x, (0, 4001, 0, 4001, 0, 200, 200, 0.7, fmt)).tobytes()
    assert len(image) % 2 == 0


def test_write_clips_and_read_wav(tmp_path):
    import torch
    x = _on_grid("s16", (3, 16000), 3)
    paths = [tmp_path / "out" / "a" / "0.wav", tmp_path / "out" / "1.wav", str(tmp_path / "2.wav")]
    got = input_data.write_clips(torch.from_numpy(x).cuda(), paths, lengths=LENGTHS)
    assert got == [str(p) for p in paths]
    for row, n in enumerate(LENGTHS):
        want = np.concatenate([x[row, :n], np.zeros(16000 - n, np.float32)])
        assert np.array_equal(input_data._read_wav(got[row], 16000), want)
        assert input_data._read_wav(got[row]).shape == (n,)


def _recording(seconds, rate, seed):
    t = np.arange(seconds * rate) / rate
    rng = np.random.default_rng(seed)
    return (0.6 * np.sin(2 * np.pi * 220 * t) + 0.2 * rng.uniform(-1, 1, t.size)).astype(np.float32)


@pytest.mark.parametrize("pad", [False, True])
def test_extract_detections(tmp_path, pad):
    import torch
    rate = 16000
    rec = _recording(5, rate, 4)
    detections = [("masiki", 300), ("masiki", 2500), ("masiki", 4900)]
    images = sa.extract_detections(detections, torch.from_numpy(rec).cuda(), sample_rate=rate, pad=pad)
    spans = [(-11200, 20800), (24000, 56000), (62400, 94400)]          # [t - 1 s, t + 1 s) in frames
    for (a, b), image in zip(spans, images):
        if pad:
            cut = np.concatenate([np.zeros(max(0, -a), np.float32), rec[max(a, 0):min(b, rec.size)], np.zeros(max(0, b - rec.size), np.float32)])
        else:
            cut = rec[max(a, 0):min(b, rec.size)]
        info, body = _body(image)
        assert (info.format, info.rate, info.frames) == ("s16", rate, cut.size) and body == ue.encode("s16", cut).tobytes()
    assert [pcm.wav_info(i).frames for i in images] == ([32000] * 3 if pad else [20800, 32000, 17600])
    # from a file at its own rate, written under dest_dir with the notebook's names
    wav = tmp_path / "stream.wav"
    wav.write_bytes(up.wav_image("s16", 1, rate, ue.encode("s16", rec).tobytes()))
    paths = sa.extract_detections(detections, wav, dest_dir=tmp_path / "extractions", target_word="masiki", pad=pad)
    assert [os.path.basename(p) for p in paths] == ["000_masiki_detection_300ms.wav", "001_masiki_detection_2500ms.wav", "002_masiki_detection_4900ms.wav"]
    assert [open(p, "rb").read() for p in paths] == images            # s16 -> float -> s16 is the identity


@pytest.mark.parametrize("include_context", [False, True])
def test_extract_shots(tmp_path, include_context):
    import torch
    rate = 16000
    rec = _recording(5, rate, 5)
    timings = [(1.0, 1.4), (0.1, 0.3), (2.0, 3.5), (4.7, 4.95), (3.00003, 3.99997)]
    d_rec = torch.from_numpy(rec).cuda()
    for fmt in ("s16", "s24"):
        images = word_extraction.extract_shots(d_rec, timings, rate=rate, include_context=include_context, format=fmt)
        for pieces, image in zip(word_extraction.shot_items(rate, rec.size, timings, include_context), images):
            info, body = _body(image)
            want = b"".join(ue.item_bytes(rec, (0, rec.size, st, nf, 0, fi, fo, 1.0, fmt)).tobytes() for st, nf, fi, fo in pieces)
            assert (info.format, info.rate, info.frames) == (fmt, rate, rate) and body == want
    assert word_extraction.extract_shots(rec, timings, rate=rate, include_context=include_context, format="s24") == images      # the host path
    paths = word_extraction.extract_shots(d_rec, timings, dests=[tmp_path / "shots" / f"{k}.wav" for k in range(5)], rate=rate,
                                          include_context=include_context, format="s24")
    assert [open(p, "rb").read() for p in paths] == images


def test_convert_clips(tmp_path):
    """Two 48 kHz files and one 16 kHz file of unequal length -> 16 kHz s16 files of each file's own converted length."""
    rng = np.random.default_rng(6)
    src, frames, rates = [], [48000, 30001, 9000], [48000, 48000, 16000]
    for k, (n, rate) in enumerate(zip(frames, rates)):
        pcm16 = (8000 * np.sin(2 * np.pi * 300 * np.arange(n) / rate) + rng.integers(-2000, 2000, n)).astype(np.int16)
        src.append(tmp_path / f"in{k}.wav")
        src[-1].write_bytes(up.wav_image("s16", 1, rate, pcm16.tobytes()))
    dests = input_data.convert_clips(src, [tmp_path / "converted" / f"out{k}.wav" for k in range(3)])
    for f, d, n, rate in zip(src, dests, frames, rates):
        want = input_data.read_wav_at(str(f), 16000)
        assert want.shape == (-(-n * 16000 // rate),)
        info, body = _body(open(d, "rb").read())
        assert (info.format, info.channels, info.rate, info.frames) == ("s16", 1, 16000, want.size)
        assert body == ue.encode("s16", want).tobytes()
    # a fixed length for all, in batches of two
    fixed = input_data.convert_clips(src, [tmp_path / "fixed" / f"out{k}.wav" for k in range(3)], desired_samples=12000, format="s24", batch=2)
    for f, d in zip(src, fixed):
        info, body = _body(open(d, "rb").read())
        assert info.frames == 12000 and body == ue.encode("s24", input_data.read_wav_at(str(f), 16000, 12000)).tobytes()
