"""-m gpu: the row-strip depthwise item of the big-image blocks (dw_strip_ in mkws_embed.hip: phase 2 of mbconv_front_kernel, P2 of
mbconv_mid_kernel) at its borders.  The item decides once per tap row and per edge column whether a read lands in the image, so the first
and last output rows and both row segments of every image size are where it can go wrong; every clip holds all of them.

Handle classes (tools/make_strip_taps_golden.py, HANDLES): one clip in a one-clip handle (front + back kernels for all of 2a-4a: the five
big-image front instantiations), 37 clips in a 40-clip handle (whole-block kernel for 2b, 3a, 4a; the two-clip 4a leaves a clip slot of its
last workgroup empty), 200 in 200 (4a with one clip per workgroup), 300 in 300, and the 40-clip handle under fuse_mid = 2 (2a and 3b as
whole blocks: the quad items) and 3.  Some clips are silent, some loud.

For the depthwise output and the block output of 2a, 2b, 3a, 3b and 4a:
  (a) they meet the float32 PyTorch-CPU oracle at the tolerances of tests/test_mid_kernel_gpu.py;
  (b) the first 3 clips equal, bit for bit, what the commit before the strip item was rewritten computed
      (tests/golden/strip_taps_parent.npz, written by tools/make_strip_taps_golden.py on that commit's library)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL = 1e-4


def _tool():
    spec = importlib.util.spec_from_file_location("make_strip_taps_golden", os.path.join(ROOT, "tools", "make_strip_taps_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _within(a, b, rtol=1e-3, floor=1e-5):
    return bool((np.abs(a - b) <= rtol * np.abs(b) + floor * np.abs(b).max()).all())


@pytest.fixture(scope="module")
def ctx(golden_dir):
    from multilingual_kws_amd import weights
    from oracle.efficientnet_oracle import BLOCKS, EmbeddingOracle
    blob = weights.synthetic_blob()
    spec = T.spectrograms()
    taps = {}

    def tap(name, t):
        if name in T.TAPS:
            taps[name] = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(T.N, -1).copy()

    oracle = EmbeddingOracle(blob)
    x = torch.as_tensor(spec).to(oracle.dtype)[:, None]
    x = oracle.stem(oracle.preprocess(x))
    for block in BLOCKS:                                          # the blocks up to 4a: nothing behind it is looked at
        x = oracle.mbconv(x, block, tap)
        if block[0] == "4a":
            break
    assert sorted(taps) == sorted(T.TAPS)
    golden = T.unpack(np.load(os.path.join(golden_dir, "strip_taps_parent.npz")))
    odd = np.zeros(T.N, dtype=bool)
    odd[list(T.SILENT + T.LOUD)] = True
    return dict(blob=blob, x=torch.from_numpy(spec).to("cuda:0"), taps=taps, golden=golden, odd=odd)


@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_strip_taps_meet_the_oracle_and_the_parent_bits(ctx, handle):
    clips = T.HANDLES[handle][1]
    got = T.run_handle(ctx["blob"], ctx["x"], handle)
    odd, ordinary = ctx["odd"][:clips], ~ctx["odd"][:clips]
    assert ordinary[:min(clips, T.GOLDEN_CLIPS)].all() and (clips < 37 or odd.sum() >= 2)
    for name in T.TAPS:
        g, exp = got[name], ctx["taps"][name][:clips]
        assert g.shape == exp.shape, (name, g.shape)
        rel_odd = _rel(g[odd], exp[odd]) if odd.any() else 0.0
        print(f"{handle} {name}: rel err ordinary {_rel(g[ordinary], exp[ordinary]):.3e}, silent / loud {rel_odd:.3e}")
        assert _rel(g[ordinary], exp[ordinary]) < REL_TOL, name
        assert rel_odd < 1e-3, name
        assert _within(g[ordinary], exp[ordinary]), name
        want = ctx["golden"][f"{handle}/{name}"]
        assert want.dtype == np.float32 and want.shape == g[:T.GOLDEN_CLIPS].shape, name
        assert np.array_equal(g[:T.GOLDEN_CLIPS], want), (name, int((g[:T.GOLDEN_CLIPS] != want).sum()))
