"""embedding/generate_stream_sentences.py on the device: compose_streams against the numpy specification on host copies, write_streams
through the WAV encoder and back, and generate_stream_and_labels from WAV files at the stream's rate and at another one."""
import math
import os

import numpy as np
import pytest

from multilingual_kws_amd import pcm
from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from multilingual_kws_amd.embedding import generate_stream_sentences as gss
from multilingual_kws_amd.embedding import input_data
from multilingual_kws_amd.embedding.generate_stream_sentences import StreamPiece
from tests.util_data import write_wav

pytestmark = pytest.mark.gpu


def _streams(to_audio, rng):
    """3 streams of 5 pieces: gaps, one overlap with a cross-fade, gains; lengths that are no multiple of anything."""
    streams = []
    for r in range(3):
        pieces = []
        for k in range(5):
            a = to_audio((rng.uniform(-0.6, 0.6, 1500 + 731 * k + 97 * r)).astype(np.float32))
            pieces.append(StreamPiece(a, is_target=k % 2 == 1, keyword=f"kw{r}", start_s=0.01 * (k + 1), end_s=0.02 * (k + 1), gain=1.0 - 0.1 * k,
                                      gap_ms=3.3 * (k == 0) + 120.0 * (k == 4), fade_ms=20.0 * (k in (2, 3)), overlap_ms=15.0 * (k == 2)))
        streams.append(pieces)
    return streams


def test_compose_streams_equals_mix_host_on_host_copies():
    import torch
    bed_np = np.random.default_rng(1).uniform(-0.3, 0.3, 4321).astype(np.float32)
    on_dev = _streams(lambda a: torch.from_numpy(a).cuda(), np.random.default_rng(0))
    on_host = _streams(lambda a: a, np.random.default_rng(0))
    audio, lengths, offsets, labels, gains = gss.compose_streams(on_dev, background=torch.from_numpy(bed_np).cuda(), bed_gain=[0.5, 0.25, 2.0],
                                                                 bed_start=[0, 4320, 10000])
    want, w_lengths, w_offsets, w_labels, w_gains = gss.compose_streams(on_host, background=bed_np, bed_gain=[0.5, 0.25, 2.0],
                                                                        bed_start=[0, 4320, 10000], device="cpu")
    assert audio.is_cuda and audio.dtype == torch.float32 and isinstance(want, np.ndarray)
    assert lengths == w_lengths and offsets == w_offsets and labels == w_labels and gains.cpu().numpy().tolist() == w_gains.tolist()
    assert offsets == [0, lengths[0], lengths[0] + lengths[1]] and audio.numel() == sum(lengths)
    assert np.array_equal(audio.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.abs(want).max() == 1.0                          # the loud bed of stream 2 reaches the clip
    # the cross-fade: piece 3 starts 15 ms before piece 2 ends
    starts, n_out = gss.plan_stream([int(p.audio.shape[0]) for p in on_host[0]], on_host[0], 16000)
    assert starts[3] == starts[2] + int(on_host[0][2].audio.shape[0]) - 240 and n_out == lengths[0]
    # with snr_db the chain stays on the device and lands on the wanted ratio
    _, _, _, _, g = gss.compose_streams(on_dev, background=torch.from_numpy(bed_np).cuda(), snr_db=[0.0, 10.0, 20.0], clip=False)
    _, _, _, _, g_host = gss.compose_streams(on_host, background=bed_np, snr_db=[0.0, 10.0, 20.0], clip=False, device="cpu")
    assert np.all(np.abs(g.cpu().numpy() - g_host) <= 2.0 ** -22 * g_host) and np.all(g_host > 0)


def test_write_streams_round_trip():
    import torch
    streams = _streams(lambda a: torch.from_numpy(a).cuda(), np.random.default_rng(2))
    audio, lengths, offsets, _, _ = gss.compose_streams(streams)
    images, labels, gains = gss.write_streams(streams, format="s16")
    assert gains is None and len(images) == 3 and [len(lab) for lab in labels] == [2, 2, 2]
    host = audio.cpu().numpy()
    for image, n, o in zip(images, lengths, offsets):
        info = pcm.wav_info(image)
        assert (info.format, info.channels, info.rate, info.frames) == ("s16", 1, 16000, n)
        back = input_data.read_recording(image, 16000).cpu().numpy()
        grid = pcm.encode_host("s16", host[o:o + n]).view("<i2").astype(np.float32) / np.float32(32768)
        assert np.array_equal(back, grid)


# lengths in frames at 16 kHz: multiples of 125, so that every duration and every label time is an exact binary fraction and the
# windows' floor() lands on the word's first sample itself (in general a label is within one sample of it)
PIECES = [(4000, None), (6250, (0.125, 0.25)), (3375, None), (5125, (0.0625, 0.1875)), (2500, None)]


@pytest.mark.parametrize("file_rate", [16000, 48000])
def test_generate_stream_and_labels_from_wav_files(tmp_path, file_rate):
    rng, rate, up = np.random.default_rng(file_rate), 16000, file_rate // 16000
    clips = tmp_path / "clips"
    wav_data, pieces, lengths = [], [], []
    for k, (n, word) in enumerate(PIECES):
        x = rng.integers(-300, 300, n * up).astype(np.int16)
        if word is not None:
            x[int(word[0] * file_rate):int(word[1] * file_rate)] = 16384
        write_wav(str(clips / f"c{k}.wav"), x, rate=file_rate)
        wav_data.append(dict(mp3name_no_ext=f"c{k}", is_target=word is not None, start_s=word and str(word[0]), end_s=word and str(word[1])))
        pieces.append(StreamPiece(None, word is not None, None, word and word[0], word and word[1]))
        lengths.append(math.ceil(n * up * rate / file_rate))
    dest = tmp_path / "out"
    os.makedirs(dest)
    times = gss.generate_stream_and_labels(dest, wav_data, "mot", clips, rate=rate, label_style="csv")
    image = (dest / "streaming_test.wav").read_bytes()
    info = pcm.wav_info(image)
    assert (info.format, info.rate, info.frames) == ("s16", rate, sum(lengths))
    want_labels, want_times = gss.stream_labels(pieces, lengths, rate, "mot")
    assert times == want_times
    truth = bsa._read_groundtruth(dest / "streaming_labels.txt")
    assert truth == want_labels and len(truth) == 2
    # the harvest at the label times, nothing in front: every window begins on its word's first sample
    stream = input_data.read_recording(image, rate).cpu().numpy()
    cuts = bsa.extract_detections(truth, str(dest / "streaming_test.wav"), before_ms=0, after_ms=50)
    starts, _ = gss.plan_stream(lengths, pieces, rate)
    for cut, k in zip(cuts, (1, 3)):
        first = starts[k] + int(PIECES[k][1][0] * rate)
        got = input_data.read_recording(cut, rate).cpu().numpy()
        assert got.shape == (800,) and np.array_equal(got, stream[first:first + 800])
        if file_rate == rate:                                # the files' own samples: the plateau begins here
            assert stream[first] == 0.5 and abs(stream[first - 1]) < 0.01
        else:                                                # converted: the edge is the filter's, half way up within a sample
            assert stream[first + 8] > 0.4 and abs(stream[first - 8]) < 0.1
    with pytest.raises(AssertionError, match="exists already"):
        gss.generate_stream_and_labels(dest, wav_data, "mot", clips, rate=rate)
