"""Writes tests/golden/g711_tables.json: the 16-bit linear value of all 256 mu-law and A-law codes as the standard library's audioop
decodes them (audioop.ulaw2lin / alaw2lin, width 2).  `check()` compares the committed file with audioop wherever that module still
imports (it leaves the standard library with Python 3.13); tests/test_pcm_cpu.py calls it.

    python tests/golden/make_g711_golden.py
"""
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "g711_tables.json")


def tables():
    import audioop
    codes = bytes(range(256))
    return dict(mulaw=list(struct.unpack("<256h", audioop.ulaw2lin(codes, 2))), alaw=list(struct.unpack("<256h", audioop.alaw2lin(codes, 2))))


def check():
    """True when audioop was there and agrees with the committed file, None when it does not import; AssertionError otherwise."""
    try:
        import audioop  # noqa: F401
    except ImportError:
        return None
    with open(PATH) as fh:
        assert json.load(fh) == tables(), "tests/golden/g711_tables.json differs from audioop"
    return True


if __name__ == "__main__":
    with open(PATH, "w") as fh:
        json.dump(tables(), fh)
        fh.write("\n")
    print("wrote", PATH)
