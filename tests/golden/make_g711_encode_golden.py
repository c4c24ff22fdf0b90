"""Writes tests/golden/g711_encode.npz: the G.711 code of every 16-bit linear sample, by CPython's audioop (lin2ulaw / lin2alaw at
width 2) -- the independent side of the mu-law and A-law rules of mkws_pcm_encode (include/mkws.h).  Entry q + 32768 of `mulaw` /
`alaw` is the code of the sample q.  audioop left the standard library with Python 3.13: run this under an older one.  The tests read
the committed file and never import audioop.

  python tests/golden/make_g711_encode_golden.py"""
import os

import numpy as np


def main():
    import audioop
    linear = np.arange(-32768, 32768, dtype="<i2").tobytes()
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, "g711_encode.npz"), mulaw=np.frombuffer(audioop.lin2ulaw(linear, 2), np.uint8),
                        alaw=np.frombuffer(audioop.lin2alaw(linear, 2), np.uint8))


if __name__ == "__main__":
    main()
