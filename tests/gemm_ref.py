"""Reference side of the GEMM edge tests (test_gemm_ref_host.py, test_gpu_gemm_edges.py); nothing here touches a GPU.

  * a restatement of gemm.hip's host route (launch_prec, launch_256, launch_tile, launch_pair, aligned_walk_sm) for the
    default environment - no GAVA_* switch set - that names the instantiation a call reaches;
  * a restatement of the persistent kernels' tile walk (my_tiles_, tile_coords; plain and ALIGN): per workgroup, its tiles;
  * an fp64 reference of every epilogue on the 16-bit-rounded operands, with optional MUTATIONS (the bugs the checks must
    catch);
  * the value regimes, two of them EXACT: with them the kernel's result is determined bit for bit;
  * the bound for the regimes that are not exact;
  * the case tables of the GPU test, which follow the dispatch tables and the walks, not the workload's shapes.

Exact regimes
  ints    A and W hold integers in [-8, 8] (exact in bf16 and fp16), bias / residual / pos / time hold integers.  Every
          product and every partial sum is an integer below 2^24 (K <= 3072: |sum| <= 64 * 2 * 3072 + bias + residual), so the
          fp32 accumulation is exact in ANY summation order and an fp32 output must equal the fp64 reference; a 16-bit
          output is ONE round-to-nearest-even of that exact value (common.h converts with plain casts).  The bias of the
          16-bit epilogues spans +-3000 so that results need that rounding (an fp16 integer is exact up to 2048, a bf16 one up
          to 256) - truncation differs there.  The folding producers use [-2, 2]: then sum x^2 over 256 columns stays an
          integer below 2^24 as well (asserted on the reference).
  onehot  row m of A is 1 at column (7 m + 3) mod K, else 0; W holds multiples of 1/64 with 8 significant bits, the bias
          multiples of 1/4: out[m, n] = W[n, k(m)] (+ W_lo[n, k(m)]) + bias[n] + resid[m, n] exactly, which pins the row,
          the column and the k index of every element separately.

The bound elsewhere (randn, offset, tiny, qgelu_tails), per element, no whole-tensor norm anywhere:
      |got - ref| <= e_out |ref| + ACC mag (+ floor)
  mag = |A| . |W|^T + |bias| + |resid| in fp64, ACC = 2^-18 (the project's constant of tests/test_gpu_train_ops.py: 64 fp32
  units of the largest possible partial sum), e_out = one rounding to nearest of the output type (2^-11 fp16, 2^-8 bf16,
  2^-24 fp32), floor = 2^-25 for fp16 outputs only (half the spacing of the fp16 subnormals).  The QuickGELU epilogues add the
  term derived at qgelu_terms().
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

F16, BF16 = 0, 1                                  # hip.PREC_F16 / hip.PREC_BF16
DTYPE = {F16: torch.float16, BF16: torch.bfloat16}
EPS = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
PREC_NAME = {F16: "f16", BF16: "bf16"}
AUTO, K256, PAIR, PP = 0, 3, 4, 5                 # hip.KERNEL_*
KERNEL_NAME = {AUTO: "auto", K256: "k256", PAIR: "pair", PP: "pp"}
H16, QGELU, F32, PATCH, QGELU_BWD = 0, 1, 2, 3, 4  # hip.EPI_*
EPI_NAME = {H16: "H16", QGELU: "H16_QGELU", F32: "F32", PATCH: "F32_PATCH", QGELU_BWD: "H16_QGELU_BWD"}
ACC = 2.0 ** -18
F64 = torch.float64
N_PATCHES, PATCH_T = 16, 3                        # the patch epilogue's frame geometry in every case here
SCALE = 0.125                                     # EPI_H16: the first N / 2 columns are scaled (q rows of a qkv GEMM)
TAILS = [s * v for v in (0.0, 1e-3, 1.0, 5.0, 20.0, 60.0, 200.0) for s in (1.0, -1.0)]

# M N K; epi; prec; kernel; avail = workgroups the persistent launch may use (0: the whole device); resid 0 | 1 in place |
# 2 from another buffer with a wider ldr; bias; split; fold 0 | "stats" | "partials"; producer 0 | 1 (x16 + row sums per 64
# columns) | 2 (rowsum_reduced); w_lo; pad 0 | 1 (lda, ldw, ldo wider than the rows); regime; aux_out (EPI_H16_QGELU)
Case = namedtuple("Case", "M N K epi prec kernel avail resid bias split fold producer w_lo pad regime aux_out",
                  defaults=(0, 0, 0, True, False, 0, 0, 0, 0, "ints", False))


def case_id(c):
    s = f"{c.M}x{c.N}x{c.K}-{EPI_NAME[c.epi]}-{PREC_NAME[c.prec]}-{KERNEL_NAME[c.kernel]}-wg{c.avail}-{c.regime}"
    for flag, name in ((c.resid, f"res{c.resid}"), (not c.bias, "nobias"), (c.split, "split"), (c.fold, f"fold_{c.fold}"),
                       (c.producer, f"prod{c.producer}"), (c.w_lo, f"wlo{c.w_lo}"), (c.pad, "pad"), (c.aux_out, "aux")):
        if flag:
            s += "-" + name
    return s


def seed_of(c):
    return (c.M * 7919 + c.N * 31 + c.K * 17 + c.epi * 5 + c.prec * 3 + c.kernel + c.avail * 13 + c.resid + len(c.regime)) % (2 ** 31)


def out_is_f32(c):
    return c.epi in (F32, PATCH)


def e_out(c):
    return 2.0 ** -24 if out_is_f32(c) else EPS[c.prec]


# ---------------------------------------------------------------------------------------------------------------------
# the host route (gemm.hip: launch_prec, launch_256, launch_tile, launch_pair), default environment
Grid = namedtuple("Grid", "tiles_m tiles_n sn sm blocks align BM")
EINVAL = "EINVAL"


def aligned_walk_sm(tiles_m, tiles_n, sn, blocks, avail):
    if blocks != avail or tiles_n % sn:
        return 0
    per_xcd = blocks // 8
    a_sm = per_xcd // sn
    if a_sm < 1:
        return 0
    units = -(-tiles_m // a_sm) * (tiles_n // sn)
    rounds_aligned = (units + 7) // 8
    rounds_plain = ((tiles_m * tiles_n + 7) // 8 + per_xcd - 1) // per_xcd
    return a_sm if rounds_aligned <= rounds_plain else 0


def cu_reserve(c, n_cu):
    """What the GPU test passes for `avail` workgroups: any reserve >= n_cu - 8 gives 8 on every device."""
    return 0 if c.avail == 0 else max(0, n_cu - c.avail)


def persistent_grid(c, n_cu=256, pair=False):
    """launch_256 / launch_pair: tile counts, super-tile, grid and walk."""
    BM = 128 if pair else 256
    tiles_m, tiles_n = -(-c.M // BM), c.N // 256
    n_tiles = tiles_m * tiles_n
    sn = min(tiles_n, 4)
    sm = min((64 if pair else 32) // sn, tiles_m)
    left = n_cu - cu_reserve(c, n_cu)
    avail = left // 8 * 8 if left > 8 else 8
    if pair:
        avail *= 2
    blocks = (n_tiles + 7) // 8 * 8 if n_tiles < avail else avail
    align = False
    if c.epi == F32 and not pair:
        a = aligned_walk_sm(tiles_m, tiles_n, sn, blocks, avail)
        if a:
            align, sm = True, a
    return Grid(tiles_m, tiles_n, sn, sm, blocks, align, BM)


def _g256(c, epi, res, split, fold, align, pp):
    return (f"{PREC_NAME[c.prec]}:g256<{EPI_NAME[epi]},RES={int(res)},SPLIT={int(split)},FOLD={int(fold)},ALIGN={int(align)},"
            f"L8=0,PP={int(pp)},HL=0>")


def _tile(c, nst):
    res = c.epi == F32 and bool(c.resid)
    split = c.epi in (H16, QGELU) and c.split
    return f"{PREC_NAME[c.prec]}:tile<128,128,{nst}><{EPI_NAME[c.epi]},RES={int(res)},SPLIT={int(split)}>"


def _launch_256(c, n_cu):
    g = persistent_grid(c, n_cu)
    aux = c.epi == QGELU_BWD
    can_pp = c.K % 128 == 0 and (2 if c.w_lo == 1 else 1) * c.K >= 256 and not c.split and not c.aux_out and not aux
    want_pp = c.kernel in (PP, AUTO)                 # GAVA_PP defaults to 1: wherever an instantiation exists
    if c.kernel == PP and not can_pp:
        return EINVAL
    fold, res = bool(c.fold), bool(c.resid)
    if want_pp and can_pp:
        if c.epi in (H16, QGELU) and fold:
            return _g256(c, c.epi, 0, 0, 1, 0, 1)
        if c.epi == H16:
            return _g256(c, H16, 0, 0, 0, 0, 1)
        if c.epi == F32:
            return _g256(c, F32, res, 0, 0, g.align, 1)
        if c.epi == PATCH:
            return _g256(c, PATCH, 0, 0, 0, 0, 1)
        if c.kernel == PP:
            return EINVAL
    if c.epi in (H16, QGELU):
        if fold:
            return EINVAL if c.split else _g256(c, c.epi, 0, 0, 1, 0, 0)
        return _g256(c, c.epi, 0, c.split, 0, 0, 0)
    if c.epi == F32:
        return _g256(c, F32, res, 0, 0, g.align, 0)
    if c.epi == PATCH:
        return _g256(c, PATCH, 0, 0, 0, 0, 0)
    return _g256(c, QGELU_BWD, 0, 0, 0, 0, 0)


def ld_of(c, cols):
    return cols + (8 if c.pad else 0)


def route(c, n_cu=256):
    """Name of the instantiation gava_gemm launches for the case (w_lo <= 1, no 16-bit residual pair, A given), or EINVAL."""
    lda, ldw = ld_of(c, c.K), ld_of(c, (2 if c.w_lo == 1 else 1) * c.K)
    if c.N % 128 or c.K % 64 or c.M <= 0:
        return EINVAL
    if c.w_lo and (c.kernel == PAIR or c.epi == QGELU_BWD):
        return EINVAL
    if c.split and c.epi not in (H16, QGELU):
        return EINVAL
    if c.fold and (c.epi not in (H16, QGELU) or c.bias):
        return EINVAL
    if c.fold == "partials" and (c.split or c.K > 1024 or c.K < 256 or c.N % 256):
        return EINVAL
    if c.producer and c.epi != F32:
        return EINVAL
    if c.producer == 2 and (c.N % 256 or c.N > 1024):
        return EINVAL
    if c.aux_out and (c.epi != QGELU or c.split):
        return EINVAL
    fits = (c.M + 256) * lda < 2 ** 31 and c.N * ldw < 2 ** 31
    can_pair = (not c.w_lo and c.epi == F32 and c.N % 256 == 0 and c.N <= 1024 and c.K % 128 == 0 and fits
                and (c.producer == 2 or not c.producer))
    if c.kernel == PAIR:
        return f"{PREC_NAME[c.prec]}:pair" if can_pair else EINVAL
    if c.kernel in (K256, PP):
        return _launch_256(c, n_cu) if c.N % 256 == 0 and fits else EINVAL
    if c.kernel != AUTO:
        return EINVAL
    if c.producer == 2 or c.fold == "partials":
        return _launch_256(c, n_cu) if c.N % 256 == 0 and fits else EINVAL
    if c.M <= 2048:
        return _tile(c, 4)
    tiles256 = -(-c.M // 256) * (c.N // 256)
    if c.epi == PATCH:
        on_256 = c.N % 256 == 0 and fits and tiles256 >= 512
    else:
        on_256 = c.N >= 1536 or (c.K >= 2048 and tiles256 >= 512) or (c.epi == F32 and tiles256 >= 512)
    if c.N % 256 == 0 and fits and on_256:
        return _launch_256(c, n_cu)
    return _tile(c, 2)


def all_instantiations():
    """Every instantiation launch_prec, launch_256 and launch_pair can launch in the default environment for w_lo <= 1, no
    16-bit residual pair, A given - written out by name, so that a new one in gemm.hip without a case fails the host test."""
    g256 = [(H16, 0, 0, 1, 0, 1), (QGELU, 0, 0, 1, 0, 1), (H16, 0, 0, 0, 0, 1),                       # the ping-pong loop
            (F32, 1, 0, 0, 1, 1), (F32, 1, 0, 0, 0, 1), (F32, 0, 0, 0, 1, 1), (F32, 0, 0, 0, 0, 1), (PATCH, 0, 0, 0, 0, 1),
            (H16, 0, 0, 1, 0, 0), (H16, 0, 1, 0, 0, 0), (H16, 0, 0, 0, 0, 0),                           # the default loop
            (QGELU, 0, 0, 1, 0, 0), (QGELU, 0, 1, 0, 0, 0), (QGELU, 0, 0, 0, 0, 0),
            (F32, 1, 0, 0, 1, 0), (F32, 0, 0, 0, 1, 0), (F32, 1, 0, 0, 0, 0), (F32, 0, 0, 0, 0, 0),
            (PATCH, 0, 0, 0, 0, 0), (QGELU_BWD, 0, 0, 0, 0, 0)]
    tile = [(H16, 0, 0), (H16, 0, 1), (QGELU, 0, 0), (QGELU, 0, 1), (F32, 1, 0), (F32, 0, 0), (PATCH, 0, 0), (QGELU_BWD, 0, 0)]
    names = []
    for prec in (F16, BF16):
        p = PREC_NAME[prec]
        names += [f"{p}:g256<{EPI_NAME[e]},RES={r},SPLIT={s},FOLD={f},ALIGN={a},L8=0,PP={pp},HL=0>" for e, r, s, f, a, pp in g256]
        names += [f"{p}:tile<128,128,{nst}><{EPI_NAME[e]},RES={r},SPLIT={s}>" for nst in (4, 2) for e, r, s in tile]
        names.append(f"{p}:pair")
    return names


N_INSTANTIATIONS = 2 * (20 + 16 + 1)


# ---------------------------------------------------------------------------------------------------------------------
# the persistent kernels' walk (gemm256_kernel / gemm_pair_kernel: my_tiles_, tile_coords)
def walk(g):
    """Per workgroup of the grid, the (m-tile, n-tile) pairs it computes, in its order."""
    n_tiles = g.tiles_m * g.tiles_n
    per_xcd = g.blocks >> 3
    ranges = -(-g.tiles_m // g.sm)
    n_chunks = g.tiles_n // g.sn if g.align else 1
    n_units = ranges * n_chunks if g.align else n_tiles
    q, r = n_units >> 3, n_units & 7
    out = []
    for b in range(g.blocks):
        xcd, slot = b & 7, b >> 3
        x_first = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        x_count = q + 1 if xcd < r else q
        my = (x_count - slot + per_xcd - 1) // per_xcd if slot < x_count else 0
        if g.align:
            sm_last = g.tiles_m - (ranges - 1) * g.sm
            if slot >= g.sm * g.sn:
                my = 0
            elif slot >= sm_last * g.sn:
                my = max(0, min(x_count, n_units - n_chunks - x_first))
            else:
                my = x_count
        tiles = []
        for j in range(my):
            if g.align:
                unit = x_first + j
                mr, ch = divmod(unit, n_chunks)
                first_m = mr * g.sm
                sm = min(g.sm, g.tiles_m - first_m)
                tiles.append((first_m + slot % sm, ch * g.sn + slot // sm))
            else:
                wg = x_first + slot + j * per_xcd
                per_group = g.sm * g.tiles_n
                grp = wg // per_group
                first_m = grp * g.sm
                sm = min(g.sm, g.tiles_m - first_m)
                w = wg - grp * per_group
                chunk, rr = divmod(w, sm * g.sn)
                tiles.append((first_m + rr % sm, chunk * g.sn + rr // sm))
        out.append(tiles)
    return out


def walk_classes(g):
    """The walk branches a grid runs through (the row labels of the issue's table)."""
    w = walk(g)
    per = [len(t) for t in w]
    tags = {f"tiles/wg={max(per)}"}
    if min(per) == 0:
        tags.add("idle workgroups")
    if len(set(per)) > 1:
        tags.add("uneven")
    ranges = -(-g.tiles_m // g.sm)
    if g.align:
        tags.add(f"aligned sm={g.sm}")
        if g.tiles_m - (ranges - 1) * g.sm < g.sm:
            tags.add("aligned short last m-range")
        if g.tiles_n // g.sn > 1:
            tags.add("aligned two column chunks")
    else:
        tags.add("plain")
        if g.tiles_n % g.sn:
            tags.add("plain tiles_n % sn")
        if g.tiles_m % g.sm:
            tags.add("plain short last m-group")
    return tags


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def out_rows(c):
    return c.M // N_PATCHES * (N_PATCHES + 1) if c.epi == PATCH else c.M


def _randint(shape, lo, hi, g, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).to(torch.float32)


def make_inputs(c, device="cpu"):
    """The operands of a case in its regime: A [M][K] and W [N][K or 2K] as views of buffers whose pad columns hold NaN."""
    g = torch.Generator(device=device).manual_seed(seed_of(c))
    dt, M, N, K = DTYPE[c.prec], c.M, c.N, c.K
    Kw = 2 * K if c.w_lo == 1 else K
    rn = lambda shape, s=1.0: torch.randn(shape, generator=g, device=device) * s
    h16_out = not out_is_f32(c)
    bias = resid = aux = pos = tim = None
    if c.regime == "ints":
        r = 2 if c.producer else 8
        A, W = _randint((M, K), -r, r, g, device), _randint((N, Kw), -r, r, g, device)
        bias = _randint((N,), -3000, 3000, g, device) if h16_out else _randint((N,), -64, 64, g, device)
        resid = _randint((M, N), -(30 if c.producer else 1000), 30 if c.producer else 1000, g, device)
        pos, tim = _randint((N_PATCHES + 1, N), -16, 16, g, device), _randint((PATCH_T, N), -16, 16, g, device)
    elif c.regime == "onehot":
        A = torch.zeros(M, K, device=device)
        rows = torch.arange(M, device=device)
        A[rows, (7 * rows + 3) % K] = 1.0
        W = _randint((N, Kw), -127, 127, g, device) / 64
        bias = _randint((N,), -40, 40, g, device) / 4
        resid = _randint((M, N), -1000, 1000, g, device) / 8
        pos, tim = _randint((N_PATCHES + 1, N), -16, 16, g, device) / 4, _randint((PATCH_T, N), -16, 16, g, device) / 4
    else:
        W = rn((N, K), K ** -0.5)
        if c.w_lo == 1:
            W = torch.cat([W, rn((N, K), K ** -0.5 * 2.0 ** -9)], 1)
        bias, resid = rn((N,), 0.5), rn((M, N))
        pos, tim = rn((N_PATCHES + 1, N)), rn((PATCH_T, N))
        if c.regime == "randn":
            A = rn((M, K)) + (0.4 if c.fold else 0.0)             # the folded consumers: a stream with a mean
        elif c.regime == "offset":
            A = 8.0 + rn((M, K))
        elif c.regime == "tiny":                                  # 2^-18 ... 2^-13: fp16 subnormals and small normals; W of order 1
            e = torch.randint(14, 19, (M, K), generator=g, device=device).to(torch.float32)
            A = torch.exp2(-e) * (1 + torch.rand((M, K), generator=g, device=device)) * torch.sign(rn((M, K)))
            W = rn((N, Kw))
            bias, resid = torch.zeros(N, device=device), torch.zeros(M, N, device=device)
        elif c.regime == "qgelu_tails":                           # the bias steps the pre-activations over both saturation ends
            A = rn((M, K), 0.05)
            bias = torch.tensor(TAILS, device=device).repeat(-(-N // len(TAILS)))[:N].contiguous()
        else:
            raise ValueError(c.regime)
    x = SimpleNamespace()
    x.A_buf = torch.full((M, ld_of(c, K)), float("nan"), dtype=dt, device=device)
    x.W_buf = torch.full((N, ld_of(c, Kw)), float("nan"), dtype=dt, device=device)
    x.A_buf[:, :K], x.W_buf[:, :Kw] = A.to(dt), W.to(dt)
    x.A, x.W = x.A_buf[:, :K], x.W_buf[:, :Kw]
    x.bias = bias.contiguous() if c.bias and not c.fold else None
    x.resid = resid if c.resid else None
    x.pos, x.time = (pos, tim) if c.epi == PATCH else (None, None)
    x.aux = None
    if c.epi == QGELU_BWD:           # kept pre-activations: the sign change of qgelu' (x ~ -0.75), both saturation ends, exact zeros
        a = rn((M, N), 2.0) + 0.3
        f = a.view(-1)
        f[::5] = torch.linspace(-13.0, 13.0, f[::5].numel(), device=device)
        f[2::13] = 0.0
        x.aux = a.to(dt)
    x.stats = x.part = x.fs = x.ft = None
    if c.fold:                       # A is the un-normalised stream x16; its row statistics as the producer would leave them
        a64 = x.A.to(F64)
        Mp = -(-M // 256) * 256
        mean = a64.mean(1)
        rstd = ((a64 - mean[:, None]).pow(2).mean(1) + 1e-5).rsqrt()
        x.stats = torch.zeros(Mp + 32, 2, device=device)
        x.stats[:M, 0], x.stats[:M, 1] = mean.float(), rstd.float()
        x.part = torch.zeros(Mp + 32, 4, 2, device=device)
        for sl in range(-(-K // 256)):
            seg = a64[:, sl * 256:(sl + 1) * 256]
            x.part[:M, sl, 0], x.part[:M, sl, 1] = seg.sum(1).float(), (seg * seg).sum(1).float()
        x.fs = x.W.to(F64).sum(1).float().contiguous()
        x.ft = (bias if c.regime == "qgelu_tails" else rn((N,), 0.3)).contiguous()
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 reference, with mutations
MUTATIONS = ("drop_k", "double_k", "swap16", "bias_neighbour", "resid_twice", "row_shift", "truncate", "last_tile_is_first")


def qgelu64(v):
    return v * torch.sigmoid(1.702 * v)


def qgelu_grad64(v):
    s = torch.sigmoid(1.702 * v)
    return s * (1 + 1.702 * v * (1 - s))


def mutated_tile(c):
    """The one tile a mutation hits: the last (ragged) m-tile, the first n-tile.  Everything else stays right - a wrong tile
    must not hide behind the others."""
    bm, bn = (128, 128) if route(c).find("tile<") >= 0 else ((128, 256) if c.kernel == PAIR else (256, 256))
    m0 = (c.M - 1) // bm * bm
    return slice(m0, c.M), slice(0, min(bn, c.N))


def pre_activation(c, x, mutation=None):
    """(v, mag): acc + bias (+ residual, + the fold) in fp64 before the epilogue's function, and the magnitude of the bound."""
    A, W = x.A.to(F64), x.W.to(F64)
    K = c.K
    if c.w_lo == 1:
        acc = A @ W[:, :K].t() + A @ W[:, K:].t()
        mag = A.abs() @ (W[:, :K].abs() + W[:, K:].abs()).t()
    else:
        acc, mag = A @ W.t(), A.abs() @ W.abs().t()
    rows, cols = mutated_tile(c)
    if mutation in ("drop_k", "double_k"):
        ks = slice(64 * ((K // 64) // 2), 64 * ((K // 64) // 2) + 64)
        acc[rows, cols] += (-1 if mutation == "drop_k" else 1) * (A[rows, ks] @ W[cols, ks].t())
    if c.fold:
        if c.fold == "stats":
            mean, rstd = x.stats[:c.M, 0].to(F64), x.stats[:c.M, 1].to(F64)
        else:
            slots = -(-K // 256)
            mean = x.part[:c.M, :slots, 0].to(F64).sum(1) / K
            rstd = (x.part[:c.M, :slots, 1].to(F64).sum(1) / K - mean * mean + 1e-5).rsqrt()
        v = rstd[:, None] * (acc - mean[:, None] * x.fs.to(F64)) + x.ft.to(F64)
        mag = rstd[:, None] * (mag + mean.abs()[:, None] * x.fs.to(F64).abs()) + x.ft.to(F64).abs()
        return v, mag
    v = acc
    if x.bias is not None:
        b = x.bias.to(F64).expand(c.M, c.N).clone()
        if mutation == "bias_neighbour":
            b[rows, cols] = torch.roll(x.bias.to(F64), -1)[cols]
        v = v + b
        mag = mag + x.bias.to(F64).abs()
    if x.resid is not None:
        r = x.resid.to(F64)
        v = v + r
        mag = mag + r.abs()
        if mutation == "resid_twice":
            v[rows, cols] += r[rows, cols]
    return v, mag


def reference(c, x, mutation=None):
    """name -> fp64 tensor of every output of the case, exact (before the rounding to the output type); "mag" and "pre" ride
    along for the bound."""
    v, mag = pre_activation(c, x, mutation)
    ref = {"mag": mag, "pre": v}
    if c.epi == H16:
        v = v.clone()
        v[:, :c.N // 2] *= SCALE
        ref["mag"] = mag.clone()
        ref["mag"][:, :c.N // 2] *= SCALE
        ref["out"] = v
    elif c.epi == QGELU:
        ref["out"] = qgelu64(v)
        if c.aux_out:
            ref["aux_out"] = v
    elif c.epi == QGELU_BWD:
        ref["out"] = v * qgelu_grad64(x.aux.to(F64))
    elif c.epi == PATCH:
        frames = c.M // N_PATCHES
        f = torch.arange(frames, device=v.device)
        ref["out"] = (v.view(frames, N_PATCHES, c.N) + x.pos[1:].to(F64)[None] + x.time.to(F64)[f % PATCH_T][:, None]).reshape(c.M, c.N)
        ref["mag"] = mag + (x.pos[1:].to(F64).abs()[None] + x.time.to(F64).abs()[f % PATCH_T][:, None]).reshape(c.M, c.N)
    else:
        ref["out"] = v
    if mutation == "swap16":
        rows, cols = mutated_tile(c)
        o = ref["out"]
        a, b = o[rows, 16:32].clone(), o[rows, 32:48].clone()
        o[rows, 16:32], o[rows, 32:48] = b, a
    if c.producer:
        w = 64 if c.producer == 1 else 256
        xs = ref["out"].view(c.M, c.N // w, w)
        ref["rowsum"] = torch.stack([xs.sum(2), (xs * xs).sum(2)], 2)
        ref["rowsum_abs"] = torch.stack([xs.abs().sum(2), (xs * xs).sum(2)], 2)
    return ref


def truncate_to(v, dt):
    """fp64 -> 16-bit type by dropping mantissa bits (the `truncate` mutation), where .to() rounds to nearest even: a rounded
    value that grew in magnitude steps back by one in its sign-magnitude bit pattern."""
    r = v.float().to(dt)
    over = r.to(F64).abs() > v.abs()
    return (r.view(torch.int16) - over.to(torch.int16)).view(dt)


def ideal_outputs(c, x, ref, mutation=None):
    """What a kernel that rounds once, correctly, would leave: name -> tensor in the output type (unpadded).  The split output is
    (hi, lo); the producer's x16 is the 16-bit copy of the fp32 output.  `truncate` replaces the rounding of 16-bit outputs."""
    dt = DTYPE[c.prec]
    to16 = (lambda t: truncate_to(t, dt)) if mutation == "truncate" else (lambda t: t.float().to(dt))
    got = {}
    if out_is_f32(c):
        got["out"] = ref["out"].float()
        if c.producer:
            got["x16"] = to16(got["out"].to(F64))
            w = 64 if c.producer == 1 else 256
            xs = got["out"].to(F64).view(c.M, c.N // w, w)
            got["rowsum"] = torch.stack([xs.sum(2), (xs * xs).sum(2)], 2).float()
    elif c.split:
        hi = to16(ref["out"])
        got["hi"], got["lo"] = hi, to16(ref["out"].float().to(F64) - hi.to(F64))
    else:
        got["out"] = to16(ref["out"])
        if c.aux_out:
            got["aux_out"] = to16(ref["aux_out"])
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the checks
EXACT_REGIMES = ("ints", "onehot")


def is_exact(c, name):
    """Outputs whose value the exact regimes determine bit for bit: everything linear.  QuickGELU and its derivative are not
    (hardware exp2 / rcp), the folded consumers are not (rstd, fs are rounded)."""
    if c.regime not in EXACT_REGIMES or c.fold or c.epi == QGELU_BWD:
        return False
    if c.epi == QGELU:
        return name == "aux_out"
    if name == "rowsum":
        return c.regime == "ints"
    return True


def qgelu_terms(pre, y):
    """The QuickGELU epilogues' own error, per element, for y = x sigma(1.702 x) evaluated in fp32 as
    x * rcp(1 + exp2(t)), t = fl(x * c), c = fl(-1.702 log2 e)  (common.h quick_gelu8).  Returns (slope, rel):

      slope  the pre-activation's error dx (accumulation, bias add) reaches y times |d/dx x sigma(1.702 x)|, whose maximum is
             1.0998 (at 1.702 x = 2.3994): slope = 1.1, applied to dx by the caller.
      rel    relative to |y|:
             * exp2 and rcp of the hardware at one ulp each: 2^-23 + 2^-23, the exp2's reaching sigma = 1 / (1 + e) with the
               factor e / (1 + e) = 1 - sigma <= 1;
             * the add 1 + e and the final multiply x * sigma, one rounding each: 2^-24 + 2^-24;
               together 3 * 2^-23;
             * the rounding of t: t = x * c carries the multiply's 2^-24 and the constant's 2^-24, |dt| <= 2^-23 |t|, and
               d sigma / dt = -ln 2 sigma (1 - sigma): relative to y, ln 2 |t| (1 - sigma) 2^-23.  For x > 0 it vanishes with
               1 - sigma; for x < 0 it grows like |t| while y itself vanishes like exp(-1.702 |x|).
    Where exp2 saturates (t > 128: inf, rcp gives 0, y = -0; t < -126: 0, y = x) the true y is within 2^-126 |x| of that."""
    x = pre
    sig = torch.sigmoid(1.702 * x)
    t = x.abs() * 2.4554669595930157
    rel = 3 * 2.0 ** -23 + math.log(2.0) * t * (1 - sig) * 2.0 ** -23
    return 1.1, rel * y.abs()


def bound(c, ref, name):
    """The per-element bound of output `name` (see the module docstring)."""
    mag, r = ref["mag"], ref[name if name not in ("hi", "lo", "sum") else "out"]
    floor = 2.0 ** -25 if (c.prec == F16 and not out_is_f32(c)) else 0.0
    eo = e_out(c)
    if name == "sum":                 # hi + lo of the split output: the fp32 value up to lo's own rounding
        eo = 2.0 ** -24 + EPS[c.prec] ** 2
    # the folded-LayerNorm consumers: the constants of gemm_check in tests/test_gpu_train_ops.py, eps |ref| + 2 eps mag
    acc_term = 2 * EPS[c.prec] * mag if c.fold else ACC * mag
    if c.epi == QGELU and name in ("out", "hi", "sum"):
        slope, own = qgelu_terms(ref["pre"], r)
        return eo * r.abs() + slope * (acc_term + 2.0 ** -24 * ref["pre"].abs()) + own + floor
    return eo * r.abs() + acc_term + floor


def rowsum_bound(c, ref):
    """(sum x, sum x^2) over w columns from the kernel's fp32 x: n additions in some order, each within 2^-24 of its partial sum
    (<= sum |x|): w 2^-24 sum |x|; the squares carry one more rounding each."""
    w = 64 if c.producer == 1 else 256
    a = ref["rowsum_abs"]
    return torch.stack([w * 2.0 ** -24 * a[..., 0], (w + 1) * 2.0 ** -24 * a[..., 1]], 2) + 1e-30


def compare(c, x, ref, got):
    """[(name, kind, value, where)]: kind "exact" -> number of differing elements, kind "ratio" -> worst error / bound.  The
    case passes when every exact value is 0 and every ratio <= 1.  NaN or inf in an output gives an infinite ratio."""
    dt = DTYPE[c.prec]
    res = []

    def one(name, g, want64, bnd):
        if is_exact(c, name):
            want = want64.float() if g.dtype == torch.float32 else want64.float().to(dt)
            bad = ~((g == want) | (torch.isnan(g) & torch.isnan(want)))
            n = int(bad.sum())
            where = ""
            if n:
                i = torch.nonzero(bad)[0].tolist()
                where = f"first at {i}: got {g[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}"
            res.append((name, "exact", n, where))
        else:
            err = (g.to(F64) - want64).abs()
            rat = torch.where(err == 0, torch.zeros_like(err), err / bnd)
            rat = torch.where(torch.isfinite(rat), rat, torch.full_like(rat, float("inf")))
            k, idx = int(rat.argmax()), []
            for n_ in reversed(rat.shape):
                k, i_ = divmod(k, n_)
                idx.insert(0, i_)
            res.append((name, "ratio", float(rat.max()), f"at {idx}"))

    if c.split:
        one("hi", got["hi"], ref["out"], bound(c, ref, "hi"))
        if is_exact(c, "lo"):
            one("lo", got["lo"], ref["out"] - got["hi"].to(F64), None)
        else:
            one("sum", got["hi"].to(F64) + got["lo"].to(F64), ref["out"], bound(c, ref, "sum"))
    else:
        one("out", got["out"], ref["out"], bound(c, ref, "out"))
    if c.aux_out:
        one("aux_out", got["aux_out"], ref["aux_out"], EPS[c.prec] * ref["aux_out"].abs()
            + (2 * EPS[c.prec] if c.fold else ACC) * ref["mag"] + (2.0 ** -25 if c.prec == F16 else 0.0))
    if c.producer:
        # the copy is the kernel's own fp32 output rounded once; the sums are taken from that fp32 output
        n = int((got["x16"] != got["out"].to(dt)).sum())
        res.append(("x16", "exact", n, ""))
        if is_exact(c, "rowsum"):
            one("rowsum", got["rowsum"], ref["rowsum"], None)
        else:
            w = 64 if c.producer == 1 else 256
            xs = got["out"].to(F64).view(c.M, c.N // w, w)
            own = torch.stack([xs.sum(2), (xs * xs).sum(2)], 2)
            one("rowsum", got["rowsum"].reshape(c.M, -1), own.reshape(c.M, -1), rowsum_bound(c, ref).reshape(c.M, -1))
    if c.epi == QGELU and c.regime == "qgelu_tails":
        g, r = got["hi" if c.split else "out"].to(F64), ref["out"]
        bad = ~torch.isfinite(g) | (g * r < 0) | ((r.abs() > 1e-3) & (torch.signbit(g) != torch.signbit(r)))
        res.append(("finite and signed", "exact", int(bad.sum()), ""))
    return res


def passes(results):
    return all((v == 0) if kind == "exact" else (v <= 1) for _, kind, v, _ in results)


def worst(results):
    return max([v for _, kind, v, _ in results if kind == "ratio"], default=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
RAGGED = (1, 129, 255)


def m_of(tiles_m, i, BM=256):
    """M with `tiles_m` m-tiles and a ragged last one (1, 129 or 255 rows of it by turns)."""
    return BM * (tiles_m - 1) + RAGGED[i % 3] * BM // 256


# (tiles_m, tiles_n, workgroups): the issue's table, each row checked against walk_classes in the host test
ALIGNED_GRIDS = [(9, 1, 8), (9, 4, 32),                      # sm = 1, two tiles on some workgroups
                 (17, 1, 16), (17, 2, 32), (25, 3, 64),      # sm = 2, short last m-range, two tiles per workgroup
                 (5, 8, 32)]                                 # two column chunks
PLAIN_GRIDS = [(3, 5, 8), (2, 9, 8), (3, 6, 16),             # tiles_n no multiple of sn
               (9, 4, 8), (11, 3, 8),                        # short last m-group (9 x 4: five tiles per workgroup)
               (3, 3, 8),                                    # the forward's N = 768
               (3, 3, 16)]                                   # 9 tiles on 16 workgroups: idle ones
# (kernel, K, w_lo): the minimum and minimum + 1 k-tile counts of each loop
LOOPS = [(K256, 64, 0), (K256, 128, 0), (K256, 192, 0), (PP, 256, 0), (PP, 384, 0), (PP, 128, 1)]


def _walk_cases():
    out = []
    for gi, (tm, tn, wg) in enumerate(ALIGNED_GRIDS):
        for li, (kern, K, w_lo) in enumerate(LOOPS):
            for prec in (F16, BF16):
                i = gi + li + prec
                out.append(Case(m_of(tm, i), 256 * tn, K, F32, prec, kern, wg, resid=i % 3, bias=i % 2 == 0, w_lo=w_lo,
                                regime="onehot" if li in (1, 4) else "ints", pad=int(i % 4 == 0)))
    for gi, (tm, tn, wg) in enumerate(PLAIN_GRIDS):
        for li, (kern, K, w_lo) in enumerate(LOOPS):
            for prec in (F16, BF16):
                i = gi + li + prec
                epi = H16 if (gi + li) % 2 == 0 else F32
                out.append(Case(m_of(tm, i), 256 * tn, K, epi, prec, kern, wg, resid=(i % 3 if epi == F32 else 0), w_lo=w_lo,
                                regime="onehot" if li in (0, 3) else "ints", pad=int(i % 4 == 1)))
    return out


def _regime_cases():
    """The regimes that are not exact, on one aligned and one plain grid with two tiles per workgroup, both loops."""
    out = []
    for regime in ("randn", "offset", "tiny"):
        for prec in (F16, BF16):
            out.append(Case(m_of(9, 0), 256, 64, F32, prec, K256, 8, resid=0 if regime == "tiny" else 1, regime=regime))
            out.append(Case(m_of(9, 1), 1024, 256, F32, prec, PP, 32, resid=0 if regime == "tiny" else 2, regime=regime))
            out.append(Case(m_of(3, 2), 1280, 192, H16, prec, K256, 8, regime=regime))
            out.append(Case(m_of(9, 0), 1024, 384, H16, prec, PP, 8, regime=regime, pad=1))
            out.append(Case(m_of(3, 1), 768, 128, H16, prec, PP, 8, w_lo=1, regime=regime))
    # deep K on few rows: the accumulation term of the bound at its largest
    out += [Case(513, 256, 3072, F32, prec, kern, 8, resid=1, regime=r) for prec in (F16, BF16) for kern in (K256, PP)
            for r in ("ints", "offset")]
    return out


def _epilogue_cases():
    out = []
    for prec in (F16, BF16):
        for regime in ("ints", "onehot", "randn"):
            # KERNEL_256 with split_out (H16 and QuickGELU); no test launched these instantiations before
            out.append(Case(m_of(3, 0), 768, 128, H16, prec, K256, 8, split=True, regime=regime))
            if regime != "onehot":
                out.append(Case(m_of(3, 1), 768, 64, QGELU, prec, K256, 8, split=True, regime=regime))
            # EPI_F32_PATCH on a given patch matrix, default loop and ping-pong, two and three tiles per workgroup
            out.append(Case(16 * 16 * 16 - 16 * 5, 256, 192, PATCH, prec, K256, 8, regime=regime))
            out.append(Case(16 * 16 * 24 - 16 * 9, 256, 256, PATCH, prec, PP, 8, regime=regime))
        # QuickGELU: plain, with the pre-activation copy, the tails; two tiles per workgroup
        for regime in ("ints", "randn", "qgelu_tails"):
            out.append(Case(m_of(2, 2), 2304, 64, QGELU, prec, K256, 8, aux_out=True, regime=regime))
            out.append(Case(m_of(16, 0), 256, 192, QGELU, prec, K256, 8, regime=regime, pad=1))
        out.append(Case(m_of(3, 0), 768, 128, QGELU, prec, K256, 8, split=True, regime="qgelu_tails"))
        # QuickGELU' dgrad epilogue, two tiles per workgroup
        out.append(Case(m_of(16, 1), 256, 128, QGELU_BWD, prec, K256, 8, bias=False, regime="randn"))
        out.append(Case(m_of(3, 2), 1536, 64, QGELU_BWD, prec, K256, 8, bias=False, regime="randn", pad=1))
    return out


def _fold_cases():
    """The folded-LayerNorm consumers with 1, 2 and 3 tiles on a workgroup (the fold block is indexed by tile parity), both
    statistics forms, the default loop and the ping-pong loop, fold_partials at its limits K = 256 and K = 1024; and the
    folding producers with the same tile counts at the minimum K of each loop (rowsum_reduced flushes a tile's sums in the
    NEXT tile's first stage: at one k-tile per tile that stage is also the last)."""
    out = []
    for prec in (F16, BF16):
        for ti, tm in enumerate((8, 16, 24)):
            for fold in ("stats", "partials"):
                for kern in (K256, PP):
                    K = 1024 if (fold == "partials" and tm == 16) else 256
                    epi = QGELU if (ti + (kern == PP)) % 2 else H16
                    out.append(Case(m_of(tm, ti), 256, K, epi, prec, kern, 8, bias=False, fold=fold, regime="randn"))
            out.append(Case(m_of(tm, ti), 256, 128, H16, prec, K256, 8, bias=False, fold="stats", regime="randn"))
            out.append(Case(m_of(tm, ti), 256, 256, QGELU, prec, K256, 8, bias=False, fold="stats", regime="qgelu_tails", aux_out=True))
            for kern, K in ((K256, 64), (PP, 256)):
                out.append(Case(m_of(tm, ti + 1), 256, K, F32, prec, kern, 8, resid=1, producer=2, regime="ints"))
                out.append(Case(m_of(tm, ti + 1), 256, K, F32, prec, kern, 8, resid=2, producer=1, regime="randn"))
        out.append(Case(m_of(3, 0), 768, 128, F32, prec, K256, 8, resid=1, producer=2, regime="ints"))       # plain walk, three slots
        out.append(Case(m_of(3, 0), 768, 256, F32, prec, PP, 8, resid=1, producer=2, regime="randn"))
    return out


def _tile_cases():
    """The 128^2 kernel: ring depth 4 | 2 on either side of M = 2048, every epilogue form on both; M = 1, 127, 128, 129."""
    out = []
    for prec in (F16, BF16):
        for M in (2048, 2049):
            out += [Case(M, 128, 64, H16, prec, regime="ints"), Case(M, 128, 128, H16, prec, split=True, regime="onehot"),
                    Case(M, 128, 64, QGELU, prec, regime="randn", aux_out=True), Case(M, 128, 64, QGELU, prec, split=True, regime="qgelu_tails"),
                    Case(M, 128, 192, F32, prec, resid=1, regime="ints", pad=1), Case(M, 128, 64, F32, prec, regime="onehot"),
                    Case(2048 if M == 2048 else 2064, 128, 64, PATCH, prec, regime="ints"),
                    Case(M, 128, 64, QGELU_BWD, prec, bias=False, regime="randn")]
        out += [Case(M, 384, 64, F32, prec, resid=2, regime="ints", pad=1) for M in (1, 127, 128, 129)]
        out += [Case(M, 128, 128, H16, prec, regime="onehot") for M in (1, 129)]
    return out


def _pair_cases():
    """The pair kernel (128 x 256 tiles, grid 2 * avail) with 2 and 3 tiles per workgroup."""
    out = []
    for prec in (F16, BF16):
        out.append(Case(m_of(32, 0, 128), 256, 128, F32, prec, PAIR, 8, resid=1, regime="ints"))           # 32 tiles on 16 workgroups
        out.append(Case(m_of(16, 1, 128), 768, 256, F32, prec, PAIR, 8, resid=2, regime="onehot", pad=1))  # 48 tiles: three each
        out.append(Case(m_of(48, 2, 128), 256, 128, F32, prec, PAIR, 8, resid=1, producer=2, regime="ints"))
        out.append(Case(m_of(16, 0, 128), 512, 384, F32, prec, PAIR, 8, resid=0, regime="randn"))
    return out


WALKS, REGIMES, EPILOGUES, FOLDS, TILE128, PAIRS = (_walk_cases(), _regime_cases(), _epilogue_cases(), _fold_cases(),
                                                    _tile_cases(), _pair_cases())
TABLES = {"walks": WALKS, "regimes": REGIMES, "epilogues": EPILOGUES, "folds": FOLDS, "tile128": TILE128, "pair": PAIRS}
ALL_CASES = [c for t in TABLES.values() for c in t]


def family(c):
    return next(name for name, t in TABLES.items() if c in t)


def siblings(c):
    """The other kernels that take the same call with the same k order: their outputs must be bit-identical."""
    if c.kernel not in (K256, PP, PAIR):
        return []
    out = []
    for k in (K256, PP, PAIR):
        if k != c.kernel and route(c._replace(kernel=k)) != EINVAL:
            out.append(k)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what lies outside an output, and the two mutations that act on the stored output
def untouched_violations(buf, rows, cols, rows_written=None):
    """Number of elements outside [0, rows) x [0, cols) of a NaN-poisoned output buffer that no longer hold the poison;
    rows_written (a bool mask over the first `rows` rows) names rows inside that must stay untouched too (the CLS rows of the
    patch epilogue's output)."""
    n = int((~torch.isnan(buf[rows:])).sum()) + int((~torch.isnan(buf[:rows, cols:])).sum())
    if rows_written is not None:
        n += int((~torch.isnan(buf[:rows][~rows_written])).sum())
    return n


def mutate_outputs(c, got, mutation):
    """`last_tile_is_first`: a workgroup with two or more tiles computes its first tile again instead of its last, whose
    outputs are then never written (they keep the poison)."""
    assert mutation == "last_tile_is_first"
    g = persistent_grid(c, pair=c.kernel == PAIR)
    tm, tn = next(t for t in walk(g) if len(t) >= 2)[-1]
    rows, cols = slice(tm * g.BM, min(c.M, (tm + 1) * g.BM)), slice(tn * 256, (tn + 1) * 256)
    out = {}
    for name, t in got.items():
        t = t.clone()
        if t.dim() == 2 and t.shape == (c.M, c.N):
            t[rows, cols] = float("nan")
        out[name] = t
    return out
