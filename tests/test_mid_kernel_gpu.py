"""-m gpu: the whole-block kernel of the big-image blocks (mbconv_mid_kernel: 2b, 3a and 4a by default, 2a and 3b with fuse_mid = 2) at the
edges of its own phases: handles of 40, 200 and 300 clips (4a packs two clips per workgroup, on a 256-CU device one in the 200-clip handle),
batches of 1, 2, 3 (an odd batch leaves a clip slot of the last workgroup empty) and 37 clips, one of them silent and one uniformly loud.
Depthwise output, gate and block output against the float32 PyTorch-CPU oracle at the tolerances of test_embedding_gpu.py, and bit identity
across sub-batches and permutations: the squeeze-excite sums inside the kernel have one fixed order, whatever shares the workgroup."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
REL_TOL = 1e-4
N, ORDINARY = 37, 35                      # clips 35 and 36 are the silent and the loud one
TAPS = ("block2b_dw", "block2b_gate", "block2b", "block3a_gate", "block3a", "block4a")
MID_BLOCKS = ("block2b", "block3a", "block4a")


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _within(a, b, rtol=1e-3, floor=1e-5):
    return bool((np.abs(a - b) <= rtol * np.abs(b) + floor * np.abs(b).max()).all())


@pytest.fixture(scope="module")
def ctx():
    from multilingual_kws_amd import weights
    from oracle.efficientnet_oracle import EmbeddingOracle
    blob = weights.synthetic_blob()
    rng = np.random.default_rng(31)
    spec = rng.integers(0, 670, size=(N, 49, 40)).astype(np.float32) * np.float32(10 / 256)
    spec[35] = 0.0
    spec[36] = rng.integers(500, 671, size=(49, 40)) * np.float32(10 / 256)
    taps = {}
    emb = EmbeddingOracle(blob).forward(spec, taps).numpy()
    dev = torch.device("cuda:0")
    return dict(blob=blob, spec=spec, x=torch.from_numpy(spec).to(dev), taps={k: v.reshape(N, -1) for k, v in taps.items()}, emb=emb, dev=dev)


def _check(got, exp, name):
    """The existing file's bounds: fp32-roundoff class on ordinary clips, north_star's 1e-3 on the silent / loud ones, element-wise form."""
    print(f"{name}: rel err ordinary {_rel(got[:ORDINARY], exp[:ORDINARY]):.3e}, silent / loud {_rel(got[ORDINARY:], exp[ORDINARY:]):.3e}")
    assert _rel(got[:ORDINARY], exp[:ORDINARY]) < REL_TOL, name
    assert _rel(got[ORDINARY:], exp[ORDINARY:]) < 1e-3, name
    assert _within(got[:ORDINARY], exp[:ORDINARY]), name


def _mid_stages(em, x):
    return {s: k for s, k, _ in em.profile(x, reps=1) if k.startswith("mbconv_mid_kernel<")}


@pytest.mark.parametrize("max_batch", [40, 200, 300])
def test_whole_block_kernel_taps_and_bit_identity(ctx, max_batch):
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    em = EmbeddingModel(ctx["blob"], max_batch=max_batch)
    try:
        x = ctx["x"]
        ran = _mid_stages(em, x)
        assert all(b in ran for b in MID_BLOCKS), ran             # 2b, 3a and 4a did run on the whole-block kernel
        if torch.cuda.get_device_properties(ctx["dev"]).multi_processor_count == 256:
            assert ran["block4a"].endswith(",1,512>" if max_batch == 200 else ",2,512>"), ran
        full = {name: em.tap(x, name).reshape(N, -1) for name in TAPS}
        emb = em.forward(x)
        for name in TAPS:
            _check(full[name].cpu().numpy(), ctx["taps"][name], name)
        got = emb.cpu().numpy()
        _check(got, ctx["emb"], "embedding")
        assert _within(got, ctx["emb"])
        for b in (1, 2, 3):
            for name in TAPS:
                assert torch.equal(em.tap(x[:b], name).reshape(b, -1), full[name][:b]), (b, name)
            assert torch.equal(em.forward(x[:b]), emb[:b]), b
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(ctx["dev"])
        for name in TAPS:
            assert torch.equal(em.tap(x[perm], name).reshape(N, -1), full[name][perm]), name
        assert torch.equal(em.forward(x[perm]), emb[perm])
    finally:
        em.close()


@pytest.mark.parametrize("fuse_mid", [2, 3])
def test_other_whole_block_plans_match_the_oracle(ctx, fuse_mid):
    """fuse_mid = 2 sends 2a and 3b through the kernel as well (its quad-item instantiations), 3 leaves 2b to the front / back pair."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    em = EmbeddingModel(ctx["blob"], max_batch=40)
    try:
        em.set_option("fuse_mid", fuse_mid)
        x = ctx["x"]
        want = ("block2a", "block2b", "block3a", "block3b", "block4a") if fuse_mid == 2 else ("block3a", "block4a")
        assert sorted(_mid_stages(em, x)) == sorted(want)
        extra = ("block2a_dw", "block2a_gate", "block2a", "block3b_dw", "block3b_gate", "block3b") if fuse_mid == 2 else ()
        for name in TAPS + extra:
            _check(em.tap(x, name).reshape(N, -1).cpu().numpy(), ctx["taps"][name], name)
        _check(em.forward(x).cpu().numpy(), ctx["emb"], "embedding")
    finally:
        em.close()
