"""Writes tests/golden/strip_taps_parent.npz: the depthwise outputs and block outputs of blocks 2a-4a, first clips of every handle class of
tests/test_strip_addressing_gpu.py, as the library under MKWS_LIB (default: the in-tree build) computes them on the GPU.

    python tools/make_strip_taps_golden.py [--out tests/golden/strip_taps_parent.npz]

Run it on the commit whose results are to be pinned (the parent of a kernel change), keep the file.  The test and this tool share the
inputs (spectrograms), the handle classes (HANDLES) and the file format (pack / unpack) through this module.

Format: the handles run the same clips, so most of their taps repeat another handle's bits or miss them by an ulp or two where a
squeeze-excite sum took another order.  An array is therefore stored once, as float32, under "<handle>/<tap>"; a later array of the same tap
that equals a stored one (or its first rows: the one-clip handle) is "<handle>/<tap>@same" = that key, and one that differs is
"<handle>/<tap>@base" = that key plus "<handle>/<tap>@ulp" = the difference of the two bit patterns as 32-bit integers.  unpack() gives every
array back bit for bit."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 300
SILENT, LOUD = (35, 150), (36, 299)
GOLDEN_CLIPS = 3
BLOCKS = ("block2a", "block2b", "block3a", "block3b", "block4a")
TAPS = tuple(t for b in BLOCKS for t in (b + "_dw", b))
# name -> (max_batch, clips, fuse_mid or None)
HANDLES = {"mb1": (1, 1, None), "mb40": (40, 37, None), "mb200": (200, 200, None), "mb300": (300, 300, None),
           "mb40_fuse2": (40, 37, 2), "mb40_fuse3": (40, 37, 3)}


def spectrograms():
    """[N, 49, 40] float32 on the micro-frontend's grid (multiples of 10/256 below 670 steps); clips SILENT are zero, clips LOUD sit in
    the top quarter of the range."""
    rng = np.random.default_rng(47)
    spec = rng.integers(0, 670, size=(N, 49, 40)).astype(np.float32) * np.float32(10 / 256)
    for i in SILENT:
        spec[i] = 0.0
    for i in LOUD:
        spec[i] = rng.integers(500, 671, size=(49, 40)) * np.float32(10 / 256)
    return spec


def run_handle(blob, x, name):
    """{tap: float32 [clips, features]} of handle class `name` on the device tensor x[N, 49, 40]."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    max_batch, clips, fuse_mid = HANDLES[name]
    em = EmbeddingModel(blob, max_batch=max_batch)
    try:
        if fuse_mid is not None:
            em.set_option("fuse_mid", fuse_mid)
        return {t: em.tap(x[:clips], t).reshape(clips, -1).cpu().numpy() for t in TAPS}
    finally:
        em.close()


def pack(arrays):
    """{"<handle>/<tap>": float32 array} -> the dict np.savez_compressed stores."""
    out, stored = {}, {}                              # stored: tap -> [key of a float32 array of that tap]
    for key in sorted(arrays, key=lambda k: -len(arrays[k])):      # longest first: a shorter array compares with the first rows of a stored one
        tap = key.split("/")[1]
        arr = np.ascontiguousarray(arrays[key], dtype=np.float32)
        best = None
        for k in stored.setdefault(tap, []):
            d = arr.view(np.uint32) - out[k][:len(arr)].view(np.uint32)          # wraps: unpack() adds it back the same way
            if best is None or np.count_nonzero(d) < np.count_nonzero(best[1]):
                best = (k, d)
        if best is None:
            out[key] = arr
            stored[tap].append(key)
        elif not best[1].any():
            out[key + "@same"] = np.array(best[0])
        else:
            out[key + "@base"], out[key + "@ulp"] = np.array(best[0]), best[1].view(np.int32)
    return out


def unpack(npz):
    """The inverse of pack(): {"<handle>/<tap>": float32 array}, bit for bit."""
    out = {}
    for key in npz.files:
        if key.endswith("@same"):
            name = key[:-5]
            out[name] = npz[str(npz[key])]
        elif key.endswith("@base"):
            name = key[:-5]
            d = npz[name + "@ulp"].view(np.uint32)
            out[name] = (npz[str(npz[key])][:len(d)].view(np.uint32) + d).view(np.float32)
        elif not key.endswith("@ulp"):
            name = key
            out[name] = npz[key]
        else:
            continue
        out[name] = out[name][:HANDLES[name.split("/")[0]][1]]
    return out


def main():
    import torch
    from multilingual_kws_amd import _lib, weights
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "strip_taps_parent.npz"))
    args = ap.parse_args()
    blob = weights.synthetic_blob()
    x = torch.from_numpy(spectrograms()).to("cuda:0")
    arrays = {}
    for name in HANDLES:
        for tap, v in run_handle(blob, x, name).items():
            arrays[f"{name}/{tap}"] = v[:GOLDEN_CLIPS]
    packed = pack(arrays)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **packed)
    back = unpack(np.load(args.out))
    assert sorted(back) == sorted(arrays) and all(np.array_equal(back[k].view(np.int32), arrays[k].view(np.int32)) for k in arrays)
    kinds = [sum(k.endswith(s) for k in packed) for s in ("@same", "@base")]
    print(f"{args.out}: {len(arrays)} arrays from {_lib.LIB_PATH} ({len(arrays) - sum(kinds)} stored, {kinds[0]} repeats, {kinds[1]} ulp differences), "
          f"{os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
