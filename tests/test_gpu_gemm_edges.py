"""gava_gemm at the edges of its dispatch: the persistent 256^2 kernel's tile switch on reduced grids (cu_reserve) with 1 ... 5
tiles per workgroup, both k-loops at their minimum depth, both tile walks with their short last ranges, every epilogue
instantiation of the three kernels - against the fp64 reference of gemm_ref.py on the same 16-bit operands.  The case tables,
the regimes and the bound live there; test_gemm_ref_host.py checks on the CPU that mutated references fall outside the checks
used here and that the tables reach every instantiation the host dispatchers can launch.

Per case: the operands are drawn on the device, with NaN in the pad columns of A and W where the case pads; every output
buffer is NaN-filled, 3 rows longer and (padded cases) 8 columns wider than what the kernel owns, and what lies outside must
still be NaN afterwards.  In the regimes `ints` and `onehot` every linear output must EQUAL the reference (torch.equal on the
once-rounded fp64 value); elsewhere each element stays inside the bound.  A second launch and every other kernel that takes the
same call (KERNEL_256 | KERNEL_PP | KERNEL_PAIR: same k order) are bit-identical.

GAVA_GEMM_EDGES_RECORD=<file>: write the worst error / bound per family and output type with the case that gave it, and the
number of elements the exact regimes compared (profiles/gemm_edges_errors.txt is such a file).
"""
import os

import pytest
import torch

from gava_clip_amd import hip
import gemm_ref as gr
from test_gpu_train_ops import gemm_check, ln_mag        # the folded consumers' bound, with its constants

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("GAVA_GEMM_EDGES_RECORD")
WORST, EXACT = {}, {}
PAD_ROWS = 3
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    if RECORD and (WORST or EXACT):
        with open(RECORD, "w") as f:
            f.write("# gava_gemm edge tests: worst error / bound per family and output type (bound = 1), and the case that gave it\n")
            f.write(f"# {'family':10s} {'output':8s} {'type':5s} {'ratio':>6s}  worst case\n")
            for (fam, name, ot), (r, where) in sorted(WORST.items()):
                f.write(f"  {fam:10s} {name:8s} {ot:5s} {r:6.3f}  {where}\n")
            f.write("# exact regimes (ints, onehot): elements compared with torch.equal | elements that differ\n")
            for (fam, ot), (n, bad) in sorted(EXACT.items()):
                f.write(f"  {fam:10s} {ot:5s} {n:12d} | {bad}\n")


def note(c, results, got):
    fam, ot = gr.family(c), "f32" if gr.out_is_f32(c) else gr.PREC_NAME[c.prec]
    for name, kind, v, _ in results:
        if kind == "ratio":
            if v > WORST.get((fam, name, ot), (-1.0, ""))[0]:
                WORST[(fam, name, ot)] = (v, gr.case_id(c))
        else:
            n, bad = EXACT.get((fam, ot), (0, 0))
            EXACT[(fam, ot)] = (n + (got[name].numel() if name in got else c.M * c.N), bad + v)


def poisoned(rows, cols, dtype):
    return torch.full((rows, cols), NAN, dtype=dtype, device="cuda")


def run(c, x, kernel):
    """One launch of the case on `kernel`: name -> output (unpadded, [M][N]); asserts that nothing outside was written."""
    dt, M, N = gr.DTYPE[c.prec], c.M, c.N
    odt = torch.float32 if gr.out_is_f32(c) else dt
    rows, width = gr.out_rows(c), (3 * N if c.split else N)
    ldo = gr.ld_of(c, width)
    buf = poisoned(rows + PAD_ROWS, ldo, odt)
    out = buf[:rows, :width]
    kw = dict(epilogue=c.epi, prec=c.prec, kernel=kernel, cu_reserve=gr.cu_reserve(c, n_cus()), w_lo=c.w_lo, M=M)
    if c.resid == 1:
        buf[:M, :N] = x.resid
        kw["resid"] = out
    elif c.resid == 2:
        rbuf = poisoned(M, N + 64, torch.float32)
        rbuf[:, :N] = x.resid
        kw["resid"] = rbuf[:, :N]
    if c.epi == gr.H16:
        kw.update(scale_cols=N // 2, scale=gr.SCALE)
    if c.split:
        kw["split_out"] = True
    abuf = x16buf = rs = None
    if c.aux_out:
        abuf = poisoned(M + PAD_ROWS, ldo, dt)
        kw["aux_out"] = abuf
    if c.epi == gr.QGELU_BWD:
        aux = torch.zeros(M, ldo, dtype=dt, device="cuda")
        aux[:, :N] = x.aux
        kw.update(aux=aux, aux_prec=c.prec)
    if c.epi == gr.PATCH:
        kw.update(pos=x.pos, time=x.time, n_patches=gr.N_PATCHES, T=gr.PATCH_T)
    if c.fold:
        kw.update(fold_s=x.fs, fold_t=x.ft, **({"fold_stats": x.stats} if c.fold == "stats" else {"fold_partials": x.part}))
    if c.producer:
        x16buf = poisoned(M + PAD_ROWS, gr.ld_of(c, N), dt)
        Mp = (M + 255) // 256 * 256
        rs = torch.full((Mp + 32, 4, 2) if c.producer == 2 else (M + PAD_ROWS, N // 64, 2), NAN, device="cuda")
        kw.update(x16_out=x16buf[:M, :N], rowsum_out=rs, rowsum_reduced=c.producer == 2)
    hip.gemm(x.A, x.W, x.bias, out, **kw)
    torch.cuda.synchronize()
    got = {}
    written = None
    if c.epi == gr.PATCH:
        r = torch.arange(rows, device="cuda")
        written = r % (gr.N_PATCHES + 1) != 0                      # row 0 of every frame is the CLS token's: not this kernel's
        full = buf[:rows, :N][written]
    else:
        full = buf[:M, :width]
    assert gr.untouched_violations(buf, rows, width, written) == 0, "out: written outside its rows or columns"
    if c.split:
        got["hi"], got["lo"] = full[:, :N], full[:, N:2 * N]
        assert torch.equal(full[:, :N], full[:, 2 * N:]), "split rows are [hi | lo | hi]"
    else:
        got["out"] = full
    if c.aux_out:
        assert gr.untouched_violations(abuf, M, N) == 0, "aux_out: written outside its rows or columns"
        got["aux_out"] = abuf[:M, :N]
    if c.producer:
        assert gr.untouched_violations(x16buf, M, N) == 0, "x16_out: written outside its rows or columns"
        got["x16"] = x16buf[:M, :N]
        slots = N // (256 if c.producer == 2 else 64)
        assert torch.isnan(rs[M:]).all() and torch.isnan(rs[:M, slots:]).all(), "rowsum_out: written outside its rows or slots"
        got["rowsum"] = rs[:M, :slots]
    return got


IDS = [gr.case_id(c) for c in gr.ALL_CASES]


@pytest.mark.parametrize("c", gr.ALL_CASES, ids=IDS)
def test_gemm_edges(c):
    dev()
    n_cu = n_cus()
    name = gr.route(c, n_cu)
    assert name != gr.EINVAL
    if c.N % 256 == 0:       # the walk the fp32-output kernels take for this grid, as the library reports it
        claim = gr.persistent_grid(c._replace(epi=gr.F32), n_cu).align
        assert hip.load().gava_gemm_aligned_walk(c.M, c.N, gr.cu_reserve(c, n_cu)) == int(claim)
    x = gr.make_inputs(c, "cuda")
    ref = gr.reference(c, x)
    got = run(c, x, c.kernel)
    res = gr.compare(c, x, ref, got)
    print(f"{name}: " + ", ".join(f"{n_} {'differs ' + str(v) if k == 'exact' else 'ratio %.3f' % v} {w}" for n_, k, v, w in res))
    if RECORD:
        note(c, res, got)
    for n_, kind, v, where in res:
        if kind == "exact":
            assert v == 0, f"{n_}: {v} elements differ from the exact result; {where}"
        else:
            assert v <= 1, f"{n_}: error reaches {v:.3f} of the bound {where}"
    if c.fold and c.epi == gr.H16:       # the same outputs under ln_mag / gemm_check of test_gpu_train_ops.py, as they stand there
        y, mag = ln_mag(x.A, torch.ones(c.K, device="cuda"), torch.zeros(c.K, device="cuda"))
        assert gemm_check(gr.case_id(c), got["out"], y, mag, x.W, x.ft, gr.EPS[c.prec], scale_cols=c.N // 2, scale=gr.SCALE) <= 1
    again = run(c, x, c.kernel)
    for n_ in got:
        assert torch.equal(got[n_], again[n_]), f"{n_}: a second launch differs"
    for k in gr.siblings(c):
        other = run(c, x, k)
        for n_ in got:
            if n_ == "rowsum" and gr.PAIR in (k, c.kernel):
                continue                                  # the pair kernel sums a row's columns in its own order
            assert torch.equal(got[n_], other[n_]), f"{n_}: {gr.KERNEL_NAME[k]} differs from {gr.KERNEL_NAME[c.kernel]}"


def test_gemm_edges_reject_paths():
    """What the tables brush: named kernels and forms that take no such call are rejected, never replaced."""
    d = dev()
    dt = torch.float16
    bad = lambda: pytest.raises(hip.GavaError, match="GAVA_EINVAL")
    M, N = 600, 256
    z = lambda r, c_, t=dt: torch.zeros(r, c_, dtype=t, device=d)
    kw = dict(epilogue=hip.EPI_H16, prec=hip.PREC_F16)
    hip.gemm(z(M, 256), z(N, 256), None, z(M, N), kernel=hip.KERNEL_PP, **kw)                        # the baseline is accepted
    with bad():
        hip.gemm(z(M, 192), z(N, 192), None, z(M, N), kernel=hip.KERNEL_PP, **kw)                    # K % 128
    with bad():
        hip.gemm(z(M, 128), z(N, 128), None, z(M, N), kernel=hip.KERNEL_PP, **kw)                    # fewer than four k-tiles
    hip.gemm(z(M, 128), z(N, 256), None, z(M, N), kernel=hip.KERNEL_PP, w_lo=1, **kw)                # ... which w_lo = 1 doubles
    part, fs = torch.zeros(768 + 32, 4, 2, device=d), torch.zeros(N, device=d)
    hip.gemm(z(M, 256), z(N, 256), None, z(M, N), fold_partials=part, fold_s=fs, fold_t=fs, **kw)
    with bad():                                                                                        # split rows with fold_partials
        hip.gemm(z(M, 256), z(N, 256), None, z(M, 3 * N), fold_partials=part, fold_s=fs, fold_t=fs, split_out=True, **kw)
    pair = dict(resid16=z(M, N), resid_lo=z(M, N), x16_out=z(768, N), xlo_out=z(768, N), rowsum_out=part, rowsum_reduced=True,
                epilogue=hip.EPI_F32, prec=hip.PREC_F16)
    hip.gemm(z(M, 256), z(N, 256), None, None, **pair)
    with bad():                                                                                        # the 16-bit pair below K = 256
        hip.gemm(z(M, 128), z(N, 128), None, None, **pair)
    torch.cuda.synchronize()
