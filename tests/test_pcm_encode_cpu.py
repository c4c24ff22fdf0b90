"""The host side of the way out (multilingual_kws_amd/pcm.py's encode half, embedding/word_extraction.py, extract_detections; include/mkws.h
"Device audio encoded into WAV sample data"), no GPU needed: headers, the numpy specification against the audioop tables and against the
decoder, the geometry of shots and detections, and the host check of the items."""
import io
import os
import struct
import wave

import numpy as np
import pytest

from multilingual_kws_amd import pcm
from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding import input_data, word_extraction
from tests import util_pcm as up
from tests import util_pcm_encode as ue

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_encode.npz")
S16 = np.arange(-32768, 32768, dtype=np.int64)


def _file(fmt, rate, frames, fill=0x5A):
    nb = frames * pcm.SAMPLE_BYTES[fmt]
    return pcm.wav_header(fmt, rate, frames) + bytes([fill]) * nb + (b"\0" if nb & 1 else b"")


@pytest.mark.parametrize("fmt", pcm.FORMATS)
@pytest.mark.parametrize("frames", [0, 1, 5, 16000])
def test_wav_header_is_parsed_back(fmt, frames):
    image = _file(fmt, 22050, frames)
    head = len(pcm.wav_header(fmt, 22050, frames))
    assert head == (44 if fmt in ("u8", "s16", "s24", "s32") else 58)
    assert pcm.wav_info(image) == pcm.WavInfo(fmt, 1, 22050, head, frames, pcm.SAMPLE_BYTES[fmt])
    # exact sizes: the RIFF chunk spans the file, pad byte included; the data chunk holds the sample bytes alone
    assert struct.unpack("<I", image[4:8])[0] == len(image) - 8 and len(image) % 2 == 0
    assert struct.unpack("<I", image[head - 4:head])[0] == frames * pcm.SAMPLE_BYTES[fmt]
    assert pcm.wav_info(_file(fmt, 8000, 3)[:-1] if fmt in ("u8", "s24") else _file(fmt, 8000, 3)).frames == 3
    stereo = pcm.wav_header(fmt, 48000, 7, channels=2)
    assert pcm.wav_info(stereo + bytes(14 * pcm.SAMPLE_BYTES[fmt])) == pcm.WavInfo(fmt, 2, 48000, head, 7, 2 * pcm.SAMPLE_BYTES[fmt])


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_wav_header_is_read_by_the_wave_module(fmt):
    with wave.open(io.BytesIO(_file(fmt, 16000, 5)), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, pcm.SAMPLE_BYTES[fmt], 16000, 5)
        assert w.readframes(5) == b"\x5a" * (5 * pcm.SAMPLE_BYTES[fmt])


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_float_files_are_read_by_scipy(fmt):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    x = np.asarray([0.0, 0.25, -1.0, 1.0 / 3.0, 1e-3], np.float32)
    image = pcm.wav_header(fmt, 44100, 5) + pcm.encode_host(fmt, x).tobytes()
    rate, got = wavfile.read(io.BytesIO(image))
    assert rate == 44100 and got.dtype == (np.float32 if fmt == "f32" else np.float64) and np.array_equal(got, x.astype(got.dtype))


def test_wav_header_refuses():
    with pytest.raises(ValueError, match="unknown sample format"):
        pcm.wav_header("s12", 16000, 1)
    with pytest.raises(ValueError, match="frames = -1"):
        pcm.wav_header("s16", 16000, -1)
    with pytest.raises(ValueError, match="do not fit"):
        pcm.wav_header("f64", 16000, 1 << 29)


@pytest.mark.parametrize("fmt", ["mulaw", "alaw"])
def test_g711_equals_the_audioop_tables(fmt):
    golden = np.load(GOLDEN)[fmt]
    assert golden.shape == (65536,) and golden.dtype == np.uint8
    v = S16.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(pcm.encode_host(fmt, v), golden)
    assert np.array_equal(ue.g711_table(fmt), golden)                    # the tests' own restatement is the same function


@pytest.mark.parametrize("fmt", ["u8", "mulaw", "alaw", "s16"])
def test_decode_encode_decode_is_decode(fmt):
    """Every code of the small alphabets and every 16-bit sample: decoded by the tests' decoder (tests/util_pcm.py), encoded, decoded
    again.  Mu-law 0x7F (negative zero) comes back as 0xFF, which decodes to the same value."""
    codes = S16.astype("<i2").view(np.uint8).reshape(-1, 2) if fmt == "s16" else np.arange(256, dtype=np.uint8).reshape(-1, 1)
    first = up.sample_values(fmt, codes)
    again = pcm.encode_host(fmt, first).reshape(codes.shape)
    assert np.array_equal(up.sample_values(fmt, again).view(np.uint32), first.view(np.uint32))
    differ = np.nonzero((again != codes).any(axis=1))[0].tolist()
    assert differ == ([0x7F] if fmt == "mulaw" else [])
    assert np.array_equal(ue.encode(fmt, first).reshape(codes.shape), again)


@pytest.mark.parametrize("fmt", pcm.FORMATS)
def test_encode_host_equals_the_tests_restatement(fmt):
    rng = np.random.default_rng(pcm.FORMAT_ID[fmt])
    edge = np.asarray([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)),
                       np.inf, -np.inf, np.nan, 1e-45, -1e-40, 1e30, -1e30, 3e38, 0.5 / 128, 1.5 / 128, 2.5 / 128, -0.5 / 128, 126.5 / 128,
                       127.5 / 128, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -1.5 / 32768, 32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768,
                       0.5 / 8388608, 1.5 / 8388608, 8388606.5 / 8388608, 0.5 * 2.0 ** -31, 1.5 * 2.0 ** -31], dtype=np.float32)
    v = np.concatenate([edge, rng.uniform(-1.3, 1.3, 4000).astype(np.float32)])
    assert ue.same_bytes(fmt, pcm.encode_host(fmt, v), ue.encode(fmt, v))
    if fmt not in ("f32", "f64"):
        zero = pcm.encode_host(fmt, np.zeros(1, np.float32))
        assert np.array_equal(pcm.encode_host(fmt, np.asarray([np.nan], np.float32)), zero)             # NaN is the code of zero
        assert zero.tolist() == [ue.ZERO_CODE.get(fmt, 0)] * pcm.SAMPLE_BYTES[fmt]


def test_half_even_rounding_and_the_rails():
    s16 = lambda v: pcm.encode_host("s16", np.asarray(v, np.float32)).view("<i2").tolist()
    assert s16([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, -2.5 / 32768]) == [0, 2, 2, 0, -2, -2]
    assert s16([1.0, 32767.5 / 32768, 32767.4 / 32768, -1.0, -1.5, np.inf, -np.inf, np.nan]) == [32767, 32767, 32767, -32768, -32768, 32767, -32768, 0]
    assert pcm.encode_host("u8", np.asarray([0.5 / 128, 1.5 / 128, -1.0, 1.0, -2.0, np.nan], np.float32)).tolist() == [128, 130, 0, 255, 0, 128]
    s32 = pcm.encode_host("s32", np.asarray([1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, -2.0, np.nan, 1.5 * 2.0 ** -31], np.float32)).view("<i4")
    assert s32.tolist() == [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 128, 2 ** 31 - 1, -2 ** 31, 0, 2]
    s24 = pcm.encode_host("s24", np.asarray([1.0, -1.0, 0.5 / 8388608, 1.5 / 8388608], np.float32)).reshape(-1, 3).tolist()
    assert s24 == [[0xFF, 0xFF, 0x7F], [0, 0, 0x80], [0, 0, 0], [2, 0, 0]]


def test_extract_one_second_pins():
    f = word_extraction.extract_one_second
    assert f(0.7, 0.1, 0.4) == (0, 0.7)
    assert f(10, 4.0, 4.5) == (3.75, 4.75)
    assert f(10, 9.6, 9.9) == (9.0, 10)
    assert f(10, 0.1, 0.3) == (0, 1.0)
    assert f(1.0, 0.2, 0.4) == (0, 1.0) and f(3, 1.0, 2.5) == (1.25, 2.25)
    import multilingual_kws.embedding.word_extraction as by_path          # the drop-in path serves the same module
    assert by_path is word_extraction


@pytest.mark.parametrize("rate", [16000, 8000, 44100])
@pytest.mark.parametrize("include_context", [False, True])
def test_shot_items_always_yield_rate_frames(rate, include_context):
    rng = np.random.default_rng(rate + include_context)
    n = 10 * rate + 17
    timings = [(0.0, 0.3), (0.1, 0.4), (4.0, 4.5), (9.6, 9.9), (9.7, n / rate), (2.0, 3.0), (2.0, 3.7), (5.0, 5.0), (0.0, 0.99999), (3.3333, 3.3334)]
    timings += [(s, s + d) for s, d in zip(rng.uniform(0, 9, 40), rng.uniform(0, 1.5, 40))]
    shots = word_extraction.shot_items(rate, n, timings, include_context)
    fade = int(np.floor(0.025 * rate + 0.5))
    for (start_s, end_s), pieces in zip(timings, shots):
        assert sum(p[1] for p in pieces) == rate, (start_s, end_s, pieces)
        words = [p for p in pieces if p[2] or p[3]]
        assert len(words) == 1 and words[0][2:] == (fade, fade)
        st, nf = words[0][:2]
        if end_s - start_s < 1 and not include_context:               # the word's own span, centred, zeros around it
            s0, s1 = int(np.floor(start_s * rate + 0.5)), int(np.floor(end_s * rate + 0.5))
            assert (st, nf) == (s0, s1 - s0)
            front = sum(p[1] for p in pieces[:pieces.index(words[0])])
            assert front == (rate - nf) // 2 and all(p[0] + p[1] <= 0 for p in pieces if p is not words[0])
        else:                                                          # one window of the recording, no padding
            assert len(pieces) == 1 and nf == rate and 0 <= st and st + nf <= n
            w0, _ = word_extraction.extract_one_second(n / rate, start_s, end_s)
            assert abs(st - w0 * rate) <= 1
    # a recording shorter than a second is taken whole, as extract_one_second does
    assert word_extraction.shot_items(16000, 11200, [(0.1, 0.4)], include_context=True) == [[(0, 11200, 400, 400)]]


def _decode_file(image):
    info = pcm.wav_info(image)
    return info, up.decode_frames(info.format, info.channels, image[info.data_offset:info.data_offset + info.frames * info.frame_bytes], 0)


def test_extract_shots_on_the_host():
    rate = 16000
    rec = np.random.default_rng(3).uniform(-0.9, 0.9, 5 * rate).astype(np.float32)
    timings = [(1.0, 1.4), (0.1, 0.3), (2.0, 3.5)]
    for include_context in (False, True):
        files = word_extraction.extract_shots(rec, timings, rate=rate, include_context=include_context, format="f32")
        for pieces, image in zip(word_extraction.shot_items(rate, rec.size, timings, include_context), files):
            rows = [(0, rec.size, st, nf, 0, fi, fo, 1.0, "f32") for st, nf, fi, fo in pieces]
            info, got = _decode_file(image)
            assert (info.format, info.rate, info.frames) == ("f32", rate, rate)
            assert np.array_equal(got.view(np.uint32), np.concatenate([ue.values(rec, r) for r in rows]).view(np.uint32))
    word = word_extraction.extract_shots(rec, [(1.0, 1.4)], rate=rate, format="f32")[0]
    _, got = _decode_file(word)
    assert not got[:4800].any() and not got[11200:].any() and got[4800] == 0 and got[11199] == 0       # padding, and the fades' ends
    assert np.array_equal(got[4800 + 400:11200 - 400], rec[16000 + 400:22400 - 400])                  # untouched between the fades
    assert got[4800 + 200] == rec[16000 + 200] * np.float32(0.5)


def test_extract_detections_geometry_and_names(tmp_path):
    rate = 16000
    rec = np.random.default_rng(4).uniform(-0.9, 0.9, 5 * rate).astype(np.float32)
    detections = [("masiki", 300), ("masiki", 2500), ("masiki", 4900)]
    assert sa.detection_windows([300, 2500, 4900], rec.size, rate) == [(0, 20800), (24000, 32000), (62400, 17600)]
    assert sa.detection_windows([300, 2500, 4900], rec.size, rate, pad=True) == [(-11200, 32000), (24000, 32000), (62400, 32000)]
    assert sa.detection_windows([1001], 50000, 22050, before_ms=500, after_ms=250) == [(11047, 16537)]     # floor(ms * rate / 1000)
    assert sa.detection_windows([100], 800, 8000, before_ms=50, after_ms=500) == [(400, 400)]             # past the end: clamped
    images = sa.extract_detections(detections, rec, sample_rate=rate)
    for (a, nf), image in zip(sa.detection_windows([300, 2500, 4900], rec.size, rate), images):
        info, got = _decode_file(image)
        assert (info.format, info.channels, info.rate, info.frames) == ("s16", 1, rate, nf)
        assert image[info.data_offset:] == ue.encode("s16", rec[a:a + nf]).tobytes()
        assert np.abs(got - rec[a:a + nf]).max() <= 0.5 / 32768 + 1e-7
    padded = sa.extract_detections(detections, rec, sample_rate=rate, pad=True, format="f32")
    want = np.concatenate([np.zeros(11200, np.float32), rec[:20800]])
    assert np.array_equal(_decode_file(padded[0])[1], want)
    assert np.array_equal(_decode_file(padded[2])[1], np.concatenate([rec[62400:], np.zeros(14400, np.float32)]))
    paths = sa.extract_detections(detections, rec, dest_dir=tmp_path / "extractions", target_word="masiki", sample_rate=rate)
    assert [os.path.basename(p) for p in paths] == ["000_masiki_detection_300ms.wav", "001_masiki_detection_2500ms.wav", "002_masiki_detection_4900ms.wav"]
    assert [open(p, "rb").read() for p in paths] == images
    own = sa.extract_detections([("left", 2500)], rec, dest_dir=tmp_path / "own", sample_rate=rate, before_ms=10, after_ms=10)
    assert os.path.basename(own[0]) == "000_left_detection_2500ms.wav" and pcm.wav_info(open(own[0], "rb").read()).frames == 320
    with pytest.raises(ValueError, match="sample_rate"):
        sa.extract_detections(detections, rec)


def test_encode_wav_on_the_host_inverts_decode_wav(tmp_path):
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, (3, 1000)).astype(np.float32) / np.float32(32768.0)
    images = input_data.encode_wav(x, 16000, "s16", lengths=[1000, 999, 1])
    for row, n, image in zip(x, (1000, 999, 1), images):
        got, rate = input_data.decode_wav(image)
        assert rate == 16000 and np.array_equal(got, row[:n])
    odd = input_data.encode_wav(x[0, :5], 8000, "u8")
    assert len(odd) == 1 and len(odd[0]) == 44 + 6 and odd[0][-1] == 0 and pcm.wav_info(odd[0]).frames == 5
    paths = input_data.write_clips(x, [tmp_path / "a" / "0.wav", tmp_path / "a" / "b" / "1.wav", tmp_path / "2.wav"], lengths=[1000, 999, 1])
    assert [open(p, "rb").read() for p in paths] == images
    faded = input_data.encode_wav(x[0], 16000, "f32", fade_ms=10, gain=0.5)[0]
    rows = [(0, 1000, 0, 1000, 0, 160, 160, 0.5, "f32")]
    assert faded[58:] == ue.item_bytes(x[0], rows[0]).tobytes()
    with pytest.raises(ValueError, match="lengths"):
        input_data.encode_wav(x, lengths=[1, 2])


def test_check_encode_items_messages():
    good = (0, 100, -5, 50, 7, 3, 3, 1.0, "s24")
    cases = [
        ((0, 100, 0, 50, 0, 0, 0, 1.0, 8), "format 8"),
        ((0, 100, 0, -1, 0, 0, 0, 1.0, "s16"), "n_frames = -1"),
        ((0, 100, 0, 50, 0, -2, 0, 1.0, "s16"), "fade_in = -2"),
        ((0, 100, 0, 50, 0, 0, -3, 1.0, "s16"), "fade_out = -3"),
        ((0, -4, 0, 50, 0, 0, 0, 1.0, "s16"), "src_len = -4"),
        ((0, 100, 0, 65, 0, 0, 0, 1.0, "s16"), "n_frames = 65 above max_frames = 64"),
        ((0, 100, (1 << 61) + 1, 50, 0, 0, 0, 1.0, "s16"), "beyond"),
        ((0, 100, -(1 << 61) - 1, 50, 0, 0, 0, 1.0, "s16"), "beyond"),
        ((901, 100, 0, 50, 0, 0, 0, 1.0, "s16"), r"source \[901, 1001\) passes the source's 1000 floats"),
        ((-1, 100, 0, 50, 0, 0, 0, 1.0, "s16"), "passes the source's"),
        ((1 << 62, 1 << 62, 0, 50, 0, 0, 0, 1.0, "s16"), "passes the source's"),
        ((0, 100, 0, 50, 151, 0, 0, 1.0, "s24"), "50 frames of 3 bytes at byte 151 pass the output's 300 bytes"),
        ((0, 100, 0, 50, -1, 0, 0, 1.0, "s16"), "pass the output's"),
        ((0, 100, 0, 1, 300, 0, 0, 1.0, "u8"), "pass the output's"),
    ]
    pcm.check_encode_items(pcm.make_encode_items([good, (0, 100, 1 << 61, 64, 44, 0, 0, 1.0, "f32"), (1000, 0, 0, 0, 300, 9, 9, 1.0, "f64")]), 1000, 300, 64)
    for row, why in cases:
        with pytest.raises(ValueError, match="pcm encode item 1: .*" + why):
            pcm.check_encode_items(pcm.make_encode_items([good, row, good]), 1000, 300, 64)
    with pytest.raises(ValueError, match="pcm encode item 0"):
        pcm.encode_items_host(np.zeros(10, np.float32), pcm.make_encode_items([(0, 11, 0, 4, 0, 0, 0, 1.0, "s16")]))
    assert pcm.ENCODE_ITEM_DTYPE.itemsize == 64 and pcm.ENCODE_ITEM_DTYPE.fields["gain"][1] == 56 and pcm.ENCODE_ITEM_DTYPE.fields["format"][1] == 60
