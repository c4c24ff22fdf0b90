"""The plan of an embedding handle as a function of (max_batch, CU count): a restatement, in plain Python and without a device, of the rules
mkws_embed_create and the launchers of multilingual_kws_amd/csrc/mkws_embed.hip decide ONCE PER HANDLE.  Every rule names the C++ function it
restates.  tests/test_embed_plan_cpu.py pins the table that follows from it; tests/test_embed_handle_boundaries_gpu.py holds a device to it
(options read back, kernel names of mkws_embed_profile) on both sides of every handle size at which the plan changes.

The restatement is of the DEFAULT options of a handle on a device whose dispatch probe passed (fuse_pair == 1): launches() says which stages
do not depend on the paired / cluster kernels, for devices where it failed."""

K_WANT_WAVES = 2048          # kWantWaves
CLUSTER_MAX_BATCH = 32       # kClusterMaxBatch
CLUSTER_BUFFER_MAX_BATCH = 64
WALK_MIN_BATCH = 128
SPLITK_FLOATS_PER_CLIP = 20480

# (stage, K, N, rows per clip): the four GEMM layers launch_gemm plans on max_batch * rows
GEMM_LAYERS = (("top", 320, 1280, 4), ("dense", 1280, 2048, 1), ("dense_1", 2048, 2048, 1), ("dense_2", 2048, 1024, 1))

# keys of plan() that follow the CU count; every other key is a function of max_batch alone
CU_KEYS = ("block_tiles", "pair_mt", "mid4a_clips", "stem_walks", "stem_grid")
# keys that differ between ANY two neighbouring handle sizes: not what a plan class is made of
PER_SIZE_KEYS = ("stem_grid",)


def _cdiv(a, b):
    return (a + b - 1) // b


def block43_row_tiles(max_batch, cus):
    """block43_row_tiles(): row tiles (3 / 2 / 1 = 4 / 2 / 1 clips) per workgroup of the 4x3-image block and chain kernels."""
    if _cdiv(max_batch, 4) >= cus:
        return 3
    if _cdiv(max_batch, 2) >= cus:
        return 2
    return 1 if cus // 2 < max_batch <= cus else 2


def pair_row_tiles(max_batch, cus):
    """pair_row_tiles(): row tiles per pair of the 2x2-image paired kernels (1 = 4 clips, 2 = 8 clips)."""
    return 1 if 2 * _cdiv(max_batch, 4) <= cus else 2


def fuse_cluster(max_batch):
    """mkws_embed_create: em->fuse_cluster = max_batch <= kClusterMaxBatch (and the dispatch probe)."""
    return 1 if max_batch <= CLUSTER_MAX_BATCH else 0


def fuse_cluster_chain(max_batch):
    """mkws_embed_create: em->fuse_cluster_chain = max_batch == 1 (and fuse_cluster); cluster_chain_ok() asks the same of every launch."""
    return 1 if max_batch == 1 else 0


def cluster_buffers(max_batch):
    """mkws_embed_create: `ncl`, the cluster exchange buffers exist up to 64 clips -- what set_option("fuse_cluster", 1) needs."""
    return 1 if max_batch <= CLUSTER_BUFFER_MAX_BATCH else 0


def fuse_mid_default(max_batch):
    """mkws_embed_create: em->fuse_mid = (max_batch == 1) ? 0 : 1."""
    return 0 if max_batch == 1 else 1


def fuse_walk(max_batch):
    """run_forward, Path::Split: launch_front(..., em->fuse_walk && em->max_batch >= 128) -- block 2a's front kernel walks the channel blocks."""
    return 1 if max_batch >= WALK_MIN_BATCH else 0


def stem_grid(batch, cus):
    """run_forward: nwg = min(B, CUs) persistent workgroups of stem_block1a_kernel (here for B = max_batch)."""
    return min(batch, cus)


def pick_tile(M, K, N):
    """pick_tile(M, NTtot, KC) -> (MT, NT, split-K)."""
    NTtot, KC = _cdiv(N, 16), _cdiv(K, 16)
    if NTtot == 1:
        return (2, 1, 1)

    def waves(mt, nt, sk):
        return _cdiv(M, 16 * mt) * _cdiv(NTtot, nt) * sk

    wide = NTtot >= 64 and KC >= 64
    if wide and 1024 <= M < 2048 and waves(1, 4, 1) >= 1024:
        return (1, 4, 1)
    if wide and waves(2, 4, 1) >= 1024:
        return (2, 4, 1)
    if wide and M > 128:
        if waves(1, 4, 1) >= 1024:
            return (1, 4, 1)
        if waves(1, 2, 1) >= 1024:
            return (1, 2, 1)
        if waves(1, 2, 2) >= 1024:
            return (1, 2, 2)
    if waves(2, 2, 1) >= K_WANT_WAVES:
        return (2, 2, 1)
    if waves(1, 2, 1) >= K_WANT_WAVES:
        return (1, 2, 1)
    if KC >= 32 and waves(1, 2, 2) >= K_WANT_WAVES:
        return (1, 2, 2)
    if KC >= 64:
        return (1, 2, 4)
    return (1, 2, 1)


def gemm_plan(max_batch, K, N, rows_per_clip, pool4=False):
    """launch_gemm() of one layer at B = max_batch: ("gemv", rows, nj) or ("gemm", MT, NT, split-K)."""
    Mplan = max_batch * rows_per_clip
    KC, NTtot = _cdiv(K, 16), _cdiv(N, 16)
    # the matrix-vector kernel: handles planned for at most 4 rows (fuse_gemv is 1 on every handle; the rows decide)
    if Mplan <= 4 and KC <= 128 and NTtot >= 32 and K % 4 == 0 and (not pool4 or Mplan == 4):
        nj = _cdiv(KC, 16)
        return ("gemv", 1 if Mplan <= 1 else 4, 2 if nj <= 2 else 5 if nj <= 5 else 8)
    mt, nt, sk = pick_tile(Mplan, K, N)
    if pool4:
        sk = 1                                   # the fused average pool lives in the direct epilogue
    if sk > 1 and sk * Mplan * NTtot * 16 > SPLITK_FLOATS_PER_CLIP * max_batch:
        sk = 1                                   # no room in the handle's split-K workspace
    return ("gemm", mt, nt, sk)


def plan(max_batch, cus):
    """The default plan of a max_batch-clip handle on a cus-CU device whose dispatch probe passed."""
    bt = block43_row_tiles(max_batch, cus)
    p = {
        "block_tiles": bt,
        "pair_mt": pair_row_tiles(max_batch, cus),
        "fuse_cluster": fuse_cluster(max_batch),
        "fuse_cluster_chain": fuse_cluster_chain(max_batch),
        "cluster_buffers": cluster_buffers(max_batch),
        "fuse_mid": fuse_mid_default(max_batch),
        "fuse_walk": fuse_walk(max_batch),
        "mid4a_clips": 1 if bt == 1 else 2,      # launch_mid(.., one_clip = block_mt43 == 1, ..): block 4a's whole-block instantiation
        "stem_grid": stem_grid(max_batch, cus),
        "stem_walks": 1 if max_batch > cus else 0,      # a persistent stem workgroup walks more than one clip
    }
    # the stand-alone top conv pools (pool4) in its epilogue; with the paired chain it is that chain's last phase and this entry is not launched
    for stage, K, N, rows in GEMM_LAYERS:
        p[stage] = gemm_plan(max_batch, K, N, rows, pool4=(stage == "top"))
    return p


def plan_class(max_batch, cus):
    p = plan(max_batch, cus)
    for k in PER_SIZE_KEYS:
        del p[k]
    return p


def boundaries(cus, upto=2048):
    """[(max_batch, (changed keys ...))] for every handle size in 2 .. upto whose plan class differs from that of max_batch - 1."""
    out, prev = [], plan_class(1, cus)
    for n in range(2, upto + 1):
        cur = plan_class(n, cus)
        changed = tuple(k for k in cur if cur[k] != prev[k])
        if changed:
            out.append((n, changed))
        prev = cur
    return out


def _gemm_launches(stage, g):
    if g[0] == "gemv":
        return [[stage, "gemv_kernel<%d,%d>" % (g[1], g[2])]]
    rows = [[stage, "pw_gemm_kernel<%d,%d,false>" % (g[1], g[2])]]
    if g[3] > 1:
        rows.append([stage + "#reduce", "splitk_reduce_kernel"])
    return rows


# stages whose launches do not depend on the paired / cluster kernels (a device whose dispatch probe failed runs them all the same)
PROBE_FREE_STAGES = ("block1a", "block2a_dw", "block2a", "block2b_dw", "block2b", "block3a_dw", "block3a", "block3b_dw", "block3b", "block4a_dw", "block4a",
                     "dense", "dense#reduce", "dense_1", "dense_1#reduce", "dense_2", "dense_2#reduce")


def launches(p, batch, fuse_top=1):
    """[[stage, kernel], ...] as mkws_embed_profile names them: one forward pass of `batch` clips on a handle of plan p (route_block and the
    launchers' ProfScope names).  fuse_top = 0: the top conv + pool as a launch of its own behind the paired chain."""
    seq = [["block1a", "stem_block1a_kernel"],
           ["block2a_dw", "mbconv_front_kernel<3,2,32,1,25,20>"], ["block2a", "mbconv_back_kernel<130,96,2,512>"]]
    if p["fuse_mid"]:
        seq += [["block2b", "mbconv_mid_kernel<3,1,13,10,144,48,1,1024>"], ["block3a", "mbconv_mid_kernel<5,2,13,10,144,48,1,512>"]]
    else:
        seq += [["block2b_dw", "mbconv_front_kernel<3,1,32,2,13,10>"], ["block2b", "mbconv_back_kernel<130,144,2,512>"],
                ["block3a_dw", "mbconv_front_kernel<5,2,32,2,13,10>"], ["block3a", "mbconv_back_kernel<35,144,3,512>"]]
    seq += [["block3b_dw", "mbconv_front_kernel<5,1,32,3,7,5>"], ["block3b", "mbconv_back_kernel<35,240,3,512>"]]
    if p["fuse_mid"]:
        seq += [["block4a", "mbconv_mid_kernel<3,2,7,5,240,48,%d,512>" % p["mid4a_clips"]]]
    else:
        seq += [["block4a_dw", "mbconv_front_kernel<3,2,32,3,7,5>"], ["block4a", "mbconv_back_kernel<12,240,5,512>"]]
    top_alone = True
    if p["fuse_cluster_chain"] and batch == 1:
        seq += [["chain:4b,4c,5a,5b,5c,6a,6b,6c,6d,7a", "mbconv_cluster_chain_kernel"]]
    elif p["fuse_cluster"]:
        for name, ks, st, h, w in (("4b", 3, 1, 4, 3), ("4c", 3, 1, 4, 3), ("5a", 5, 1, 4, 3), ("5b", 5, 1, 4, 3), ("5c", 5, 1, 4, 3), ("6a", 5, 2, 4, 3),
                                   ("6b", 5, 1, 2, 2), ("6c", 5, 1, 2, 2), ("6d", 5, 1, 2, 2), ("7a", 3, 1, 2, 2)):
            seq += [["block" + name, "mbconv_cluster_kernel<%d,%d,%d,%d>" % (ks, st, h, w)]]
    else:
        seq += [["chain:4b,4c,5a,5b,5c,6a", "mbconv_chain_kernel<%d,8>" % p["block_tiles"]]]
        seq += [["chain:6b,6c,6d,7a" + (",top" if fuse_top else ""), "mbconv_pair_chain_kernel<%d,8>" % p["pair_mt"]]]
        top_alone = not fuse_top
    if top_alone:
        seq += _gemm_launches("top", p["top"])
    for stage in ("dense", "dense_1", "dense_2"):
        seq += _gemm_launches(stage, p[stage])
    return seq


def stages_that_differ(a, b):
    """The stages whose launches differ between two [[stage, kernel], ...] sequences."""
    da, db = {}, {}
    for d, seq in ((da, a), (db, b)):
        for stage, kernel in seq:
            d.setdefault(stage, []).append(kernel)
    return {s for s in set(da) | set(db) if da.get(s) != db.get(s)}


# plan keys that show in no kernel name and no option: block 2a's walk and the stem grid change a launch's grid only, and the cluster exchange
# buffers show in whether set_option("fuse_cluster", 1) succeeds
INVISIBLE_KEYS = ("fuse_walk", "stem_walks", "stem_grid", "cluster_buffers")
_TINY_STAGES = {"block" + b for b in ("4b", "4c", "5a", "5b", "5c", "6a", "6b", "6c", "6d", "7a")} | {
    "chain:4b,4c,5a,5b,5c,6a,6b,6c,6d,7a", "chain:4b,4c,5a,5b,5c,6a", "chain:6b,6c,6d,7a,top", "chain:6b,6c,6d,7a", "top"}
# the stages of launches() in which a change of the key may show
STAGES_OF_KEY = {
    "dense": {"dense", "dense#reduce"}, "dense_1": {"dense_1", "dense_1#reduce"}, "dense_2": {"dense_2", "dense_2#reduce"}, "top": {"top"},
    "block_tiles": {"chain:4b,4c,5a,5b,5c,6a"}, "mid4a_clips": {"block4a"}, "pair_mt": {"chain:6b,6c,6d,7a,top", "chain:6b,6c,6d,7a"},
    "fuse_cluster": _TINY_STAGES, "fuse_cluster_chain": _TINY_STAGES,
    "fuse_mid": {"block2b_dw", "block2b", "block3a_dw", "block3a", "block4a_dw", "block4a"},
}

# what a test taps on both sides of an edge, by the plan key that changes there
_CLUSTER_TAPS = ("block4b_dw", "block4b_gate", "block4b", "block4c", "block5a_dw", "block5a", "block5b_gate", "block5b", "block5c", "block6a_dw", "block6a_gate",
                 "block6a", "block6b_dw", "block6b_gate", "block6b", "block6c", "block6d", "block7a_dw", "block7a_gate", "block7a")
_DENSE_TAPS = ("gap", "dense", "dense_1", "dense_2")
TAPS_OF_KEY = {
    "dense": _DENSE_TAPS, "dense_1": _DENSE_TAPS, "dense_2": _DENSE_TAPS,
    "top": ("top", "gap"),
    "block_tiles": ("block4a", "block4c", "block5b_gate", "block6a"), "mid4a_clips": ("block4a",),
    "pair_mt": ("block6b", "block6d", "block7a"),
    "fuse_walk": ("block2a_dw", "block2a"),
    "fuse_cluster": _CLUSTER_TAPS, "fuse_cluster_chain": _CLUSTER_TAPS, "cluster_buffers": _CLUSTER_TAPS,
    "fuse_mid": ("block2b", "block3a", "block4a"),
    "stem_walks": ("block1a",),
}


def taps_of(changed):
    """Stage names to tap at an edge where the keys `changed` change, in network order of first mention, without repeats."""
    out = []
    for k in changed:
        for t in TAPS_OF_KEY.get(k, ()):
            if t not in out:
                out.append(t)
    return out
