"""What the frontend configuration matrix (tests/util_frontend_cases.py) is for: each branch of mkws_frontend.hip that depends on the
configuration is reached by some case.  Fails when the matrix is edited so that a branch is no longer reached.  No GPU needed: the
plan of mkws_frontend_create is restated on the CPU and tied to the library's own host tables."""
import numpy as np
import pytest

from tests.util_frontend_cases import CASES, SIGNAL_NAMES, case_signals, full_cfg, plan, stream_geometry, stream_recording

NAMES = list(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_the_restated_plan_is_the_librarys(name):
    """Scalars and filterbank tables of the restatement equal frontend.host_scalars / host_table, so the tap lists the plan is built
    from are the ones the device gets; the oracle and make_cfg both accept the configuration."""
    from multilingual_kws_amd import frontend
    from oracle.frontend_oracle import FrontendOracle
    over, n = CASES[name]
    cfg = frontend.make_cfg(**over)
    p, hs = plan(name), frontend.host_scalars(cfg)
    for k in ("window_size", "window_step", "fft_size", "start_index", "end_index", "num_weights"):
        assert p[k] == hs[k], (k, p[k], hs[k])
    assert p["fft_size"] == 512 and full_cfg(name)["num_channels"] <= 64           # what mkws_frontend_create accepts
    for k in ("weights", "unweights", "chan_freq_starts", "chan_weight_starts", "chan_widths"):
        assert np.array_equal(np.asarray(p[k], dtype=np.int16), frontend.host_table(cfg, k)), k
    fo = FrontendOracle(**over)
    for k in ("window_size", "window_step", "fft_size", "end_index"):
        assert fo.scalar(k) == p[k], k
    if p["window_size"] % 2 == 1:
        # the last sample of an odd window (load_frame's tsel == 1) meets a Hann coefficient that rounds to zero: the device cases
        # hold that load to its bounds and the lanes around it to their values; the selected value itself cannot show in any output
        assert frontend.host_table(cfg, "window_coef")[-1] == 0
    frames = frontend.num_frames(cfg, n)
    assert frames == fo.num_frames(n) == (n - p["window_size"]) // p["window_step"] + 1
    assert frames * full_cfg(name)["num_channels"] <= 3960                         # the clip kernel's LDS tile


def test_the_matrix_reaches_every_branch_it_is_meant_to():
    P = {name: plan(name) for name in NAMES}
    for name, p in P.items():
        print(name, "window", p["window_size"], "step", p["window_step"], "helped", len(p["helped"]), "len1", p["out_len"].count(1),
              "longest", max(p["out_len"]), "nm", p["nm"], "max sum", max(p["sums"]), "fast48", p["fast48"])
    fast = [p for p in P.values() if p["fast48"]]
    slow = [p for p in P.values() if not p["fast48"]]
    # the 16-bit filterbank path: every padded lane length it can have, and every helper layout
    assert {p["nm"] for p in fast} == {12, 16, 20}
    assert {0, 1, 24} <= {len(p["helped"]) for p in fast}
    assert any(1 in p["out_len"] for p in fast)                                    # a list the fast path reads past at once
    assert all(p["nm"] % 4 == 0 and p["nm"] <= 32 and max(p["sums"]) <= 65536 for p in fast)
    # the 64-bit path: for the weight sums alone, and with lanes too long for the 16-bit accumulators
    assert any(p["nm"] <= 32 and not p["sum_ok"] for p in slow)
    assert any(p["nm"] > 32 for p in slow)
    # helper lanes: none, one, 31 of 33 channels, one list split in two
    C = {name: full_cfg(name)["num_channels"] for name in NAMES}
    assert {(C[name], len(p["helped"])) for name, p in P.items()} >= {(64, 0), (63, 1), (33, 31), (1, 1), (40, 24)}
    assert max(C.values()) == 64 and any(c % 2 == 1 and c > 1 for c in C.values())  # 64 scan lanes, odd channel counts
    # odd windows (tsel == 1, unaligned loads) on each filterbank path; an odd step
    assert any(p["window_size"] % 2 == 1 for p in fast) and any(p["window_size"] % 2 == 1 for p in slow)
    assert any(p["window_step"] % 2 == 1 and p["window_size"] % 2 == 0 for p in P.values())
    # no zero padding / the live tail at its bound; a live tail of more than five steps
    assert any(p["window_size"] == 512 for p in P.values())
    assert any(p["window_size"] > 5 * p["window_step"] for p in P.values())
    # post-processing switches, each on a configuration of its own
    assert any(not full_cfg(name)["enable_log"] for name in NAMES) and any(not full_cfg(name)["enable_pcan"] for name in NAMES)
    assert len({full_cfg(name)["sample_rate"] for name in NAMES}) >= 5


def test_the_signal_set():
    for name in ("default", "sr12345"):
        pcm = case_signals(name)
        n = CASES[name][1]
        assert pcm.shape == (len(SIGNAL_NAMES), n) and pcm.dtype == np.int16
        s = dict(zip(SIGNAL_NAMES, pcm))
        assert s["noise_full"].min() < -32000 and s["noise_full"].max() > 32000 and np.abs(s["noise_amp3"]).max() == 3
        assert not s["burst"][:n // 3].any() and not s["burst"][-(n // 3):].any() and np.abs(s["burst"][n // 2 - 100:n // 2 + 100]).max() > 30000
        assert (s["const_min"] == -32768).all() and (s["const_max"] == 32767).all()
        assert s["nyquist"][:4].tolist() == [32767, -32768, 32767, -32768]
        assert s["impulses"][97] == 32767 and s["impulses"][131] == -32768 and np.count_nonzero(s["impulses"]) < n // 50
        assert 29000 < s["chirp"].max() <= 30000 and s["chirp"][0] == 0
        assert np.abs(s["quiet_loud"][:n // 2]).max() == 1 and (np.abs(s["quiet_loud"][n // 2:]) == 20000).all()
        assert not s["zeros"].any()
        assert np.array_equal(pcm, case_signals.__wrapped__(name))                 # the same clips on every call


@pytest.mark.parametrize("name", ["c64_nopcan", "sr22050_nolog", "sr11025", "w512", "w272"])
def test_the_stream_geometry(name):
    """21 frames per window, 41 windows, all four signals inside the recording; what each stream case is chosen for."""
    from multilingual_kws_amd import frontend
    p = plan(name)
    window, hop, total = stream_geometry(name)
    cfg = frontend.make_cfg(**CASES[name][0])
    assert frontend.num_frames(cfg, window) == 21 and hop == 2 * p["window_step"]
    assert frontend.live_windows(total, window, hop) == 41
    rec = stream_recording(name)
    assert rec.shape == (total,) and all(np.abs(rec[k * total // 4:(k + 1) * total // 4]).max() > 0 for k in range(4))
    want = {"c64_nopcan": full_cfg(name)["num_channels"] == 64, "sr22050_nolog": p["window_size"] % 2 == 1,
            "sr11025": p["window_step"] % 2 == 1, "w512": p["window_size"] == 512, "w272": p["window_size"] > 5 * p["window_step"]}
    assert want[name]
