"""The host side of the device WAV decode (multilingual_kws_amd/pcm.py, include/mkws.h "WAV sample data decoded on the device"), no GPU
needed: the header parser and the numpy restatement of the arithmetic (tests/util_pcm.py) against independent readers -- scipy, the
standard library's wave, the existing decode_wav -- the G.711 tables against a committed fixture, mkws_pcm_frame_bytes, the host check
of an item table, and the new keyword of every entry point."""
import inspect
import io
import json
import os
import wave

import numpy as np
import pytest

from multilingual_kws_amd import _lib, pcm
from multilingual_kws_amd.embedding import input_data
from tests import util_pcm as up

RNG = np.random.default_rng(23)


def _random_samples(fmt, frames, channels):
    if fmt in ("u8", "mulaw", "alaw"):
        return RNG.integers(0, 256, (frames, channels))
    if fmt in ("f32", "f64"):
        return RNG.uniform(-1.5, 1.5, (frames, channels))
    bits = 8 * up.SAMPLE_BYTES[fmt]
    return RNG.integers(-(1 << (bits - 1)), 1 << (bits - 1), (frames, channels))


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32", "f64"])
def test_parser_and_restatement_against_scipy_and_wave(fmt, channels):
    from scipy.io import wavfile
    frames, rate = 37, 22050
    x = _random_samples(fmt, frames, channels)
    data = up.encode(fmt, x)
    image = up.wav_image(fmt, channels, rate, data)
    info = pcm.wav_info(image)
    assert info == (fmt, channels, rate, image.index(b"data") + 8, frames, up.SAMPLE_BYTES[fmt] * channels)
    assert pcm.frame_bytes(fmt, channels) == info.frame_bytes
    assert image[info.data_offset:info.data_offset + frames * info.frame_bytes] == data
    got = np.stack([up.decode_frames(fmt, channels, data, c) for c in range(channels)], axis=1)
    # scipy: integers as they are stored (24-bit as int32 << 8), floats as floats
    srate, sx = wavfile.read(io.BytesIO(image))
    sx = sx.reshape(frames, channels)
    assert srate == rate
    if fmt == "u8":
        want = (sx.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
    elif fmt == "s16":
        want = sx.astype(np.float32) / np.float32(32768)
    elif fmt == "s24":
        assert sx.dtype == np.int32 and not (sx & 0xFF).any()
        want = (sx >> 8).astype(np.float32) / np.float32(8388608)
    elif fmt == "s32":
        want = sx.astype(np.float32) * np.float32(2.0 ** -31)
    else:
        want = sx.astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if fmt in ("u8", "s16", "s24", "s32"):             # the standard library's reader: PCM only
        with wave.open(io.BytesIO(image)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (channels, up.SAMPLE_BYTES[fmt], rate, frames)
            assert w.readframes(frames) == data
    if fmt == "s16":                                   # and the project's own 16-bit reader
        y, r = input_data.decode_wav(image)
        assert r == rate and np.array_equal(y.view(np.uint32), got[:, 0].view(np.uint32))
    # the mix: the sequential float32 sum of the channels over float32(channels)
    acc = np.zeros(frames, np.float32)
    for c in range(channels):
        acc = acc + got[:, c]
    assert np.array_equal(up.decode_frames(fmt, channels, data, "mix").view(np.uint32), (acc / np.float32(channels)).view(np.uint32))


@pytest.mark.parametrize("fmt", up.FORMATS)
def test_extensible_header(fmt):
    data = up.encode(fmt, _random_samples(fmt, 11, 6))
    plain = pcm.wav_info(up.wav_image(fmt, 6, 48000, data))
    image = up.wav_image(fmt, 6, 48000, data, extensible=True, valid_bits=8 * up.SAMPLE_BYTES[fmt] - 4)
    info = pcm.wav_info(image)
    assert info.data_offset == image.index(b"data") + 8 and info._replace(data_offset=0) == plain._replace(data_offset=0)
    with pytest.raises(ValueError, match="unknown sub-format GUID"):
        pcm.wav_info(up.wav_image(fmt, 6, 48000, data, extensible=True, guid_tail=bytes(14)))
    with pytest.raises(ValueError, match="22-byte extension"):
        short = bytearray(image)
        short[36:38] = (0).to_bytes(2, "little")       # cbSize
        pcm.wav_info(bytes(short))


def test_chunk_walk_and_sizes():
    x = _random_samples("s24", 9, 2)
    data = up.encode("s24", x)
    base = pcm.wav_info(up.wav_image("s24", 2, 44100, data))
    # an odd-sized chunk in front of data is word-padded
    odd = up.wav_image("s24", 2, 44100, data, junk=b"abcde")
    info = pcm.wav_info(odd)
    assert info.data_offset == base.data_offset + 8 + 6 and info.frames == 9 and odd[info.data_offset:info.data_offset + 54] == data
    # a streamed file: the data size is 0xFFFFFFFF and the data runs to the end of the file
    assert pcm.wav_info(up.wav_image("s24", 2, 44100, data, data_size=0xFFFFFFFF)).frames == 9
    # a trailing partial frame is dropped (4 of the 6 bytes of a tenth frame)
    assert pcm.wav_info(up.wav_image("s24", 2, 44100, data + b"\1\2\3\4")).frames == 9
    # bytes behind the data chunk are not samples
    assert pcm.wav_info(up.wav_image("s24", 2, 44100, data, tail=b"LIST\4\0\0\0abcd")).frames == 9
    assert pcm.wav_info(up.wav_image("mulaw", 1, 8000, b"")) == ("mulaw", 1, 8000, base.data_offset + 2, 0, 1)
    # bytearray and memoryview images parse too
    assert pcm.wav_info(bytearray(odd)) == info and pcm.wav_info(memoryview(odd)) == info


def test_refusals():
    data = bytes(24)
    with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
        pcm.wav_info(b"RIFX" + bytes(40))
    with pytest.raises(ValueError, match="lacks a fmt or data chunk"):
        pcm.wav_info(up.wav_image("s16", 1, 16000, data).replace(b"data", b"dat_"))
    with pytest.raises(ValueError, match="lacks a fmt or data chunk"):
        pcm.wav_info(up.wav_image("s16", 1, 16000, data).replace(b"fmt ", b"fmt_"))
    with pytest.raises(ValueError, match=r"format 1, 12 bits"):
        pcm.wav_info(up.wav_image("s16", 1, 16000, data, bits=12))
    with pytest.raises(ValueError, match=r"format 3, 16 bits"):
        pcm.wav_info(up.wav_image("s16", 1, 16000, data, code=3))
    with pytest.raises(ValueError, match=r"format 6, 16 bits"):
        pcm.wav_info(up.wav_image("s16", 1, 16000, data, code=6))
    with pytest.raises(ValueError, match=r"format 2, 4 bits"):                 # ADPCM
        pcm.wav_info(up.wav_image("u8", 1, 16000, data, code=2, bits=4))
    with pytest.raises(ValueError, match=r"format 85, 8 bits"):                # inside an extensible header as well
        pcm.wav_info(up.wav_image("u8", 1, 16000, data, code=85, extensible=True))
    with pytest.raises(ValueError, match="block_align 5 is not channels"):
        pcm.wav_info(up.wav_image("s16", 2, 16000, data, block_align=5))
    with pytest.raises(ValueError, match="0 channels"):
        pcm.wav_info(up.wav_image("s16", 0, 16000, data))
    # what the existing reader refuses is what the new one accepts
    with pytest.raises(ValueError, match="only 16-bit PCM WAV is supported"):
        input_data.decode_wav(up.wav_image("s24", 1, 16000, data))


def test_g711_tables_match_the_fixture(golden_dir):
    with open(os.path.join(golden_dir, "g711_tables.json")) as fh:
        gold = json.load(fh)
    assert len(gold["mulaw"]) == len(gold["alaw"]) == 256
    assert up.mulaw_table().tolist() == gold["mulaw"] and up.alaw_table().tolist() == gold["alaw"]
    assert (min(gold["mulaw"]), max(gold["mulaw"]), min(gold["alaw"]), max(gold["alaw"])) == (-32124, 32124, -32256, 32256)
    codes = np.arange(256, dtype=np.uint8)
    for fmt in ("mulaw", "alaw"):
        want = np.asarray(gold[fmt], np.float32) / np.float32(32768)
        assert np.array_equal(up.decode_frames(fmt, 1, codes.tobytes(), 0), want)
    from tests.golden import make_g711_golden
    assert make_g711_golden.check() in (True, None)    # None: this Python has no audioop any more


def test_frame_bytes_c_abi():
    L = _lib.lib()
    for i, fmt in enumerate(pcm.FORMATS):
        for channels in (1, 2, 3, 8, 255):
            assert L.mkws_pcm_frame_bytes(i, channels) == up.SAMPLE_BYTES[fmt] * channels == pcm.frame_bytes(fmt, channels)
    for fmt, channels in ((-1, 1), (8, 1), (0, 0), (1, -3), (5, 1 << 29)):
        assert L.mkws_pcm_frame_bytes(fmt, channels) == -1                     # MKWS_ERR_INVALID_ARG
        assert b"pcm_frame_bytes" in L.mkws_last_error()
        with pytest.raises(ValueError, match="pcm_frame_bytes"):
            pcm.frame_bytes(fmt, channels)
    with pytest.raises(ValueError):
        pcm.frame_bytes("s12", 1)
    assert pcm.ITEM_DTYPE.itemsize == 48 and [pcm.ITEM_DTYPE.fields[n][1] for n in pcm.ITEM_DTYPE.names] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert pcm.channel_index("mix") == pcm.MIX == -1 and pcm.channel_index(3) == 3
    with pytest.raises(ValueError):
        pcm.channel_index("left")


def test_host_validation_of_a_bad_table():
    import torch
    host_bytes = torch.zeros(100, dtype=torch.uint8)       # a host tensor: the table is checked before anything touches a device
    good = (4, 16, 0, 20, "s16", 3, 1)
    bad = [
        ((101, 0, 0, 4, "u8", 1, 0), "pass the buffer"),            # an offset past the bytes
        ((-1, 1, 0, 4, "u8", 1, 0), "pass the buffer"),
        ((4, 17, 0, 20, "s16", 3, 1), "pass the buffer"),           # one frame too many
        ((0, -1, 0, 4, "u8", 1, 0), "n_frames = -1"),
        ((0, 1, 0, -4, "u8", 1, 0), "out_len = -4"),
        ((0, 1, 0, 4, 8, 1, 0), "format 8"),
        ((0, 1, 0, 4, -1, 1, 0), "format -1"),
        ((0, 1, 0, 4, "u8", 0, 0), "0 channels"),
        ((0, 1, 0, 4, "s16", 2, 2), "channel 2 of 2"),
        ((0, 1, 0, 4, "s16", 2, -2), "channel -2 of 2"),
        ((0, 1, 30, 11, "u8", 1, 0), "pass the output"),            # with out_floats = 40 below
        ((0, 1, -1, 4, "u8", 1, 0), "pass the output"),
        ((0, 1, 0, 21, "u8", 1, 0), "above max_out_len"),           # with max_out_len = 20 below
    ]
    for row, why in bad:
        with pytest.raises(ValueError, match=f"pcm item 1: .*{why}"):
            pcm.decode_on_device(host_bytes, pcm.make_items([good, row, good]), out_floats=40, max_out_len=20)
    # a table that passes is stopped at the device, not before
    with pytest.raises(ValueError, match="must be on the device"):
        pcm.decode_on_device(host_bytes, pcm.make_items([good, (100, 0, 40, 0, "f64", 2, "mix")]), out_floats=40, max_out_len=20)
    with pytest.raises(ValueError, match="contiguous uint8"):
        pcm.decode_on_device(torch.zeros(8, dtype=torch.int16), pcm.make_items([good]))


def test_convert_and_channel_keywords():
    from multilingual_kws_amd import run
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
    from multilingual_kws_amd.embedding import distance_filtering as df
    from multilingual_kws_amd.embedding import transfer_learning as tl
    for fn in (tl.evaluate_files_many, tl.classification_curves, df.embed_files, df.cluster_and_sort_many, df.export_keyword_embeddings,
               input_data.AudioDataset.__init__, tl.transfer_learn, tl.transfer_learn_many):
        p = inspect.signature(fn).parameters
        assert "convert" in p and p["convert"].default is False, fn
    for fn in (sa.multi_keyword_detections, sa.multi_keyword_operating_curves, run.inference):
        p = inspect.signature(fn).parameters
        assert "channel" in p and p["channel"].default == 0 and p["resample"].default is False, fn
    for fn in (input_data.read_clips, input_data.read_recording):
        p = inspect.signature(fn).parameters
        assert p["sample_rate"].default == 16000 and p["channel"].default == 0 and p["device"].default is None, fn
    assert inspect.signature(input_data.read_clips).parameters["desired_samples"].default == 16000
    import multilingual_kws.embedding.input_data as by_path            # the drop-in path serves the same functions
    assert by_path.read_clips is input_data.read_clips and by_path.read_recording is input_data.read_recording
    # the default of AudioDataset reads nothing differently: no GPU is touched by building one without background files
    ds = input_data.AudioDataset(input_data.standard_microspeech_model_settings(3), ["x"], None, [], convert=True)
    assert ds.convert is True and ds.background_host is None
    with pytest.raises(ValueError, match="needs resample=True"):
        sa.multi_keyword_detections(["a"], [object()], "no_such.wav", channel=1)
