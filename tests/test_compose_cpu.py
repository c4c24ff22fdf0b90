"""The host side of the stream assembly (compose.py, embedding/generate_stream_sentences.py) without a GPU: the numpy specification
against the position-by-position restatement of tests/util_compose.py, the planning and label arithmetic, the table checks and the
reference's file formats."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest

from multilingual_kws_amd import _lib, compose, pcm
from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from multilingual_kws_amd.embedding import generate_stream_sentences as gss
from multilingual_kws_amd.embedding.generate_stream_sentences import StreamPiece
from tests import util_compose as uc


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("maker", uc.CASES, ids=lambda m: m.__name__[5:])
def test_mix_host_equals_the_restatement(maker):
    c = uc.get(maker)
    want, bad = c.expected
    assert bad == 0
    got = compose.mix_host(c.src, c.items, c.descs, c.bed_gain, c.clip, out=np.full(c.out_floats, uc.CANARY, np.float32))
    assert _same_bits(got, want), np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:8]


def test_power_and_gain_host_equal_the_restatement():
    c = uc.get(uc.case_beds)
    p_fg, p_bed = compose.power_host(c.src, c.items, c.descs)
    want_fg, want_bed = uc.powers(c.src, c.item_rows, c.desc_rows, c.max_out)
    assert p_fg.tolist() == want_fg.tolist() and p_bed.tolist() == want_bed.tolist()
    for snr in (-10.0, 0.0, 10.0, 30.0):
        g = compose.bed_gain_host(p_fg, p_bed, c.descs, compose.snr_scale([snr] * len(c.descs)))
        want = [np.float32(uc.gain_for(want_fg[r], want_bed[r], c.desc_rows[r]["bed_len"] > 0, snr)) for r in range(len(c.descs))]
        assert g.dtype == np.float32 and g.tolist() == want and g[-1] == 0.0 and g[-2] == 0.0       # no bed; no foreground
    # the definition: the mixed stream has the wanted ratio
    g = compose.bed_gain_host(p_fg, p_bed, c.descs, compose.snr_scale([10.0] * len(c.descs)))
    assert abs(10 * math.log10(p_fg[3] / (float(g[3]) ** 2 * p_bed[3])) - 10.0) < 1e-5


def test_struct_sizes_and_tables():
    assert compose.ITEM_DTYPE.itemsize == ctypes.sizeof(_lib.StreamItem) == 64
    assert compose.DESC_DTYPE.itemsize == ctypes.sizeof(_lib.StreamDesc) == 56
    assert compose.ITEM_DTYPE == uc.ITEM and compose.DESC_DTYPE == uc.DESC
    # rows in any order -> sorted by stream and out_start, stably; the descriptors count them and take the longest
    rows = [(0, 9, 0, 5, 30, 0, 0, 1.0, 1), (0, 9, 0, 7, 10, 0, 0, 1.0, 0), (0, 9, 0, 3, 10, 0, 0, 2.0, 1), (0, 9, 0, 4, 10, 0, 0, 3.0, 1),
            (0, 9, 0, 2, 5, 0, 0, 1.0, 0)]
    items, order = compose.make_stream_items(rows, return_order=True)
    assert order.tolist() == [4, 1, 2, 3, 0] and items["gain"].tolist() == [1.0, 1.0, 2.0, 3.0, 1.0]
    descs = compose.make_stream_descs([(0, 40, 0, 0, 0), (40, 40, 0, 0, 0), (80, 8, 0, 0, 0)], items)
    assert descs["first_item"].tolist() == [0, 2, 5] and descs["n_items"].tolist() == [2, 3, 0] and descs["max_frames"].tolist() == [7, 5, 0]
    compose.check_stream_tables(items, descs, 9, 88, 40)


def _spoilt(what, index, field, value):
    items, descs = uc.invalid_base()
    items, descs = copy.deepcopy(items), copy.deepcopy(descs)
    at = uc.spoil(items, descs, what, index, field, value)
    return uc.pack(items, uc.ITEM), uc.pack(descs, uc.DESC), at, items, descs


def test_check_stream_tables_names_every_defect():
    items, descs = uc.invalid_base()
    out_floats = descs[-1]["out_offset"] + uc.INVALID_N_OUT
    compose.check_stream_tables(uc.pack(items, uc.ITEM), uc.pack(descs, uc.DESC), uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
    for field, value in uc.BAD_ITEMS:
        t_items, t_descs, k, rows, drows = _spoilt("item", 2, field, value)
        assert not uc.item_ok(rows[k], k, drows, uc.INVALID_SRC)
        assert compose.item_problem(t_items[k], k, t_descs, uc.INVALID_SRC) is not None, (field, value)
        with pytest.raises(ValueError, match=rf"stream item {k}: "):
            compose.check_stream_tables(t_items, t_descs, uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
    for field, value in uc.BAD_STREAMS:
        t_items, t_descs, r, rows, drows = _spoilt("stream", 2, field, value)
        assert not uc.stream_ok(drows[r], len(rows), uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
        why = compose.stream_problem(t_descs[r], len(t_items), uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
        assert why is not None, (field, value)
        with pytest.raises(ValueError, match=r"stream (item \d+|2): "):
            compose.check_stream_tables(t_items, t_descs, uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
    # unordered items: valid for the kernel's check, refused by the host's
    items[3], items[4] = items[4], items[3]
    with pytest.raises(ValueError, match="stream 1: item 4 .*ascending"):
        compose.check_stream_tables(uc.pack(items, uc.ITEM), uc.pack(descs, uc.DESC), uc.INVALID_SRC, out_floats, uc.INVALID_N_OUT)
    with pytest.raises(ValueError, match="ascending"):
        compose.mix_host(np.zeros(uc.INVALID_SRC, np.float32), uc.pack(items, uc.ITEM), uc.pack(descs, uc.DESC))


def test_plan_stream_geometry():
    P = StreamPiece
    # no gaps: back to back
    assert gss.plan_stream([10, 0, 7], [P(None), P(None), P(None)], 16000) == ([0, 10, 10], 17)
    # a gap after the first piece, an overlap after the second, a gap after the last (silence at the end)
    pieces = [P(None, gap_ms=2.0), P(None, overlap_ms=1.0), P(None, gap_ms=0.5)]
    assert gss.plan_stream([100, 50, 30], pieces, 16000) == ([0, 132, 166], 204)
    # rounding at half a frame: floor(ms * rate / 1000 + 0.5)
    assert [gss.ms_to_frames(ms, 16000) for ms in (0.0, 0.03125, 0.03124, 0.09375, 1.0, 2.5)] == [0, 1, 0, 2, 16, 40]
    assert gss.ms_to_frames(0.5, 1000) == 1 and gss.ms_to_frames(1.5, 1000) == 2 and gss.ms_to_frames(0.49, 1000) == 0
    # an overlap that reaches past the whole piece is refused; an empty stream is empty
    with pytest.raises(ValueError):
        gss.plan_stream([10, 10], [P(None, overlap_ms=1.0), P(None)], 16000)
    assert gss.plan_stream([], [], 16000) == ([], 0)
    # the last piece overlapping: the stream still ends with its last sample
    assert gss.plan_stream([100, 40], [P(None, overlap_ms=5.0), P(None, overlap_ms=1.0)], 1000) == ([0, 95], 135)


LENGTHS = [33333, 20011, 47999, 16001, 12345, 31007]


def _label_pieces():
    P = StreamPiece
    return [P(None), P(None, True, "oui", 0.51, 0.93), P(None), P(None, True, "non", "0.25", "0.5"), P(None, True, None, 0.1, 0.2), P(None)]


def test_stream_labels_equal_the_reference_loop(tmp_path):
    pieces, rate = _label_pieces(), 16000
    labels, times = gss.stream_labels(pieces, LENGTHS, rate, target_word="mot")
    # the reference's loop (generate_stream_sentences.py:222-244) on the durations sox reports, frames / rate
    want_times, current = [], 0
    for p, n in zip(pieces, LENGTHS):
        duration_s = n / rate
        if not p.is_target:
            current += duration_s
            continue
        want_times.append((current + float(p.start_s), current + float(p.end_s)))
        current += duration_s
    assert times == want_times
    assert labels == [(kw, s * 1000) for kw, (s, _) in zip(("oui", "non", "mot"), want_times)]
    for style, want_lines in (("sentences", [f"mot, {s * 1000}\n" for s, _ in want_times]),
                              ("csv", [f"{kw},{s * 1000}\n" for kw, (s, _) in zip(("oui", "non", "mot"), want_times)])):
        lines = gss.label_lines(labels, "mot", style)
        assert lines == want_lines
        path = tmp_path / f"{style}.txt"
        path.write_text("".join(lines))
        back = bsa._read_groundtruth(path)
        assert [t for _, t in back] == [s * 1000 for s, _ in want_times]
        assert [k for k, _ in back] == (["mot"] * 3 if style == "sentences" else ["oui", "non", "mot"])
    # gaps and overlaps move the running time by their own frames
    pieces[0].gap_ms, pieces[2].overlap_ms = 10.0, 2.5
    _, shifted = gss.stream_labels(pieces, LENGTHS, rate)
    starts, _ = gss.plan_stream(LENGTHS, pieces, rate)
    for (s, _), k in zip(shifted, (1, 3, 4)):
        assert abs(s - (starts[k] / rate + float(pieces[k].start_s))) < 1e-9


def test_generate_stream_and_labels_on_host_arrays(tmp_path):
    rate, rng = 16000, np.random.default_rng(5)
    pieces = _label_pieces()
    audio = [(rng.uniform(-0.5, 0.5, n) * 0.01).astype(np.float32) for n in LENGTHS]
    wav_data = []
    for p, a in zip(pieces, audio):
        if p.is_target:
            a[int(round(float(p.start_s) * rate)):int(round(float(p.end_s) * rate))] = 0.5          # the word: a loud plateau
        wav_data.append(dict(wav=a, is_target=p.is_target, start_s=p.start_s, end_s=p.end_s))
    times = gss.generate_stream_and_labels(tmp_path, wav_data, "mot", rate=rate, device="cpu")
    image = (tmp_path / "streaming_test.wav").read_bytes()
    info = pcm.wav_info(image)
    assert (info.format, info.channels, info.rate, info.frames) == ("s16", 1, rate, sum(LENGTHS))
    samples = np.frombuffer(image, "<i2", info.frames, info.data_offset)
    assert np.array_equal(samples.view(np.uint8), pcm.encode_host("s16", np.concatenate(audio)))
    truth = bsa._read_groundtruth(tmp_path / "streaming_labels.txt")
    assert [k for k, _ in truth] == ["mot"] * 3 and [t for _, t in truth] == [s * 1000 for s, _ in times]
    for _, t_ms in truth:                                    # the label points at the word's first sample within one sample
        first = math.floor(t_ms * rate / 1000 + 0.5)
        assert abs(t_ms / 1000 - first / rate) <= 1 / rate
        assert samples[first] == 16384 and abs(int(samples[first - 2])) < 200
    with pytest.raises(AssertionError, match="exists already"):
        gss.generate_stream_and_labels(tmp_path, wav_data, "mot", rate=rate, device="cpu")
    # the csv style, with a bed at a given gain: the same audio bits as mix_host on the same tables
    os.makedirs(tmp_path / "b")
    bed = rng.uniform(-0.1, 0.1, 5000).astype(np.float32)
    gss.generate_stream_and_labels(tmp_path / "b", wav_data, "mot", rate=rate, format="f32", label_style="csv", background=bed, bed_gain=0.5,
                                   bed_start=4999, device="cpu")
    assert (tmp_path / "b" / "streaming_labels.txt").read_text().splitlines()[0] == f"mot,{times[0][0] * 1000}"
    image = (tmp_path / "b" / "streaming_test.wav").read_bytes()
    info = pcm.wav_info(image)
    got = np.frombuffer(image, "<f4", info.frames, info.data_offset)
    fg = np.concatenate(audio)
    want = fg + bed[(4999 + np.arange(fg.size)) % 5000] * np.float32(0.5)
    assert np.array_equal(got, np.clip(want, -1, 1))


def test_compose_streams_argument_checks():
    a = np.zeros(10, np.float32)
    with pytest.raises(ValueError, match="background"):
        gss.compose_streams([[StreamPiece(a)]], snr_db=10, device="cpu")
    with pytest.raises(ValueError, match="exactly one"):
        gss.compose_streams([[StreamPiece(a)]], background=a, device="cpu")
    with pytest.raises(ValueError, match="exactly one"):
        gss.compose_streams([[StreamPiece(a)]], background=a, snr_db=3, bed_gain=1.0, device="cpu")
    audio, lengths, offsets, labels, gains = gss.compose_streams([[StreamPiece(a)], []], device="cpu")
    assert lengths == [10, 0] and offsets == [0, 10] and labels == [[], []] and gains is None and audio.shape == (10,)


def test_module_alias():
    import multilingual_kws.embedding.generate_stream_sentences as alias
    assert alias is gss
