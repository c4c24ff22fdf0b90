"""The resampler geometries shared by tests/test_resample_cpu.py and tests/test_resample_geometries_gpu.py, and the lengths derived
from them.  A case is (name, rate_in, cfg overrides); rate_out is 16000 throughout.  What makes each case telling -- its L, M, T and the
code path that only it takes in mkws_resample.hip -- is asserted on the host alone in test_resample_cpu.py, so that an edit of this
table fails there instead of silently testing less on the device.  The emulator stays in tests/util_resample.py."""
from math import gcd

RATE_OUT = 16000
TILE = 1024                           # outputs of one workgroup (mkws_resample.hip)
HOP = 320                             # the model's hop: the output samples of a live session's smallest push
PUSHES = 12

CASES = (
    # name, rate_in, overrides                                  what it is there for
    ("equal", 16000, {}),                                       # L = M = 1
    ("down2", 32000, {}),                                       # L == 1 kernels, M = 2
    ("down6", 96000, {}),                                       # T - 1 = 384: two trips of the live kernel's history loops
    ("down12", 192000, {}),                                     # T - 1 = 768: three trips; the live kernel asks for more than 48 KB of LDS
    ("l4m3", 12000, {}),                                        # small L, up-conversion, L divides the tile
    ("l2m3", 24000, {}),                                        # L = 2 with M > L
    ("cd_half", 22050, {}),                                     # L = 320
    ("cd_quarter", 11025, {}),                                  # L = 640 > M = 441
    ("l_above_tile", 15999, {}),                                # L = 16000: the phase index never wraps inside a tile
    ("short_filter", 48000, dict(zero_crossings=1)),            # T = 7
    ("long_filter", 48000, dict(zero_crossings=64)),            # the shipped L, M with twice the taps
    ("box_window", 44100, dict(zero_crossings=3, kaiser_beta=0.0, rolloff=1.0)),   # both legal extremes
)
SHIPPED = (("ship48k", 48000, {}), ("ship44k1", 44100, {}), ("ship8k", 8000, {}))
ALL_CASES = CASES + SHIPPED
BY_NAME = {c[0]: c for c in ALL_CASES}
NAMES = tuple(c[0] for c in CASES)
ALL_NAMES = tuple(c[0] for c in ALL_CASES)
DEFAULT_FILTER_NAMES = tuple(c[0] for c in ALL_CASES if not c[2])

# L, M, T of every case of CASES, by the header's formulas (include/mkws.h, "Sample-rate conversion")
TABLE = dict(equal=(1, 1, 65), down2=(1, 2, 129), down6=(1, 6, 385), down12=(1, 12, 769), l4m3=(4, 3, 65), l2m3=(2, 3, 97),
             cd_half=(320, 441, 89), cd_quarter=(640, 441, 65), l_above_tile=(16000, 15999, 65), short_filter=(1, 3, 7),
             long_filter=(1, 3, 385), box_window=(160, 441, 17))


def factors(rate_in, rate_out=RATE_OUT):
    """-> (L, M)."""
    g = gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def live_out_samples(L):
    """The smallest multiple of L that is at least one hop: a push of that many output samples is a whole number of input samples."""
    return -(-HOP // L) * L


def short_out_samples(L, M, T):
    """The smallest legal push (L outputs from M inputs) when it brings fewer new samples than the T - 1 the state keeps, else None."""
    return L if M < T - 1 else None
