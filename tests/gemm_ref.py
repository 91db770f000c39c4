"""Float64 references, error bounds and the arena helper for the dense products (csrc/gemm_f32.hip, gemm_bf16.hip, gemm_bf16_dma.hip,
gemm_bf16_p.hip, gemm_split3.hip).  Plain numpy / torch: no library; the arena lives on whatever device it is asked for, so
tests/test_gemm_bounds_cpu.py runs all of it on the CPU and tests/test_gemm_f64_gpu.py on the GPU.

1. The activation sweep.  The product is arranged so that the accumulator is an EXACT fp32 number in every family and for every
   summation order: A [M, K] is one-hot, A[m, m % K] = s_m with s_m cycling over S_CYCLE = (0, 1, -2, 0.5), the other operand is all
   ones (exact in bf16 and as x3 pieces), so acc[m, n] = s_m.  Forward layout: bias[n] carries the sweep, the argument of the
   activation is u = fp32(s_m) + fp32(bias[n]), ONE fp32 addition that numpy restates bit for bit.  Input-gradient layout: aux_in[m, n]
   carries the sweep (row m shifted by m / M of the grid step, planted points unshifted) and the result is s_m * f(aux_in[m, n]).
   GELU and GELU' of those fp32 arguments are evaluated in float64 with Phi(x) = erfc(-x / sqrt 2) / 2 for x < 0 and
   1 - erfc(x / sqrt 2) / 2 for x >= 0: no cancellation on either side.

   Bounds, |got - ref| <= B * scale + 2^-23 |ref| (+ 2^-8 |ref| where only a bf16 output is written):
     gelu_pair_fast (epilogue 5)     B = 1.5 x 4.2e-7 for gelu and 1.5 x 3.0e-7 for gelu' (the accuracy csrc/common.h documented).  The numpy
                                     restatement with an exact reciprocal and an exact exp2 stays below them (test_gemm_bounds_cpu.py); the device's
                                     v_rcp_f32 / v_exp_f32 are ~1 ulp approximations acting on H <= 0.5, i.e. <= ~1e-7 more.
     gelu_erf, dgelu_erf (2 and 3)   B = 2^-21 max(1, |x|): OpenCL's limit for erf is 16 ulp, so Phi is off by <= 0.5 * 16 * 2^-24 =
                                     2^-21, and the error of x Phi (and of x phi) scales with |x|.
     x aux (epilogue 6)              B = 0: the product of an fp32 value with 0, 1, -2 or 0.5 is exact.
   scale is what the function's value is multiplied by before it is stored: 1 in the forward layout (C = gelu(u), aux_out =
   gelu'(u)), |s_m| in the input-gradient layout (C = s_m * gelu'(x)): a row with s_m = 0 must hold exact zeros there.
   2^-23 |ref| covers the rounding of the final product (x * Phi, s_m * gelu') at large |x|, where B alone is relative to 1.

2. The arena.  A matrix window placed inside a flat tensor: a front guard of G0 elements (4100 fp32 / 4104 bf16: the window base is
   16-byte aligned and NOT 32-byte aligned -- torch's own allocations are 512-byte aligned, the library promises 16), the window's
   elements at base + index (any index map: rows of a leading dimension ld > width, x3 pieces, k-piece slabs with a free stride)
   and a back guard (the rest of the last row and 256 ld elements more: beyond any tile's overhang).  An INPUT arena is NaN everywhere outside
   the window -- padding columns, the memory after the last row, both guards -- and no finite output may depend on those elements.
   An OUTPUT arena is pre-filled with a sentinel bit pattern (a NaN with a payload); after the call every element outside the window
   must hold that pattern bit for bit (compared on an integer view) and every element inside must have been written: none is NaN."""
import math

import numpy as np
import torch

F = np.float32
D = np.float64
ULP = 2.0 ** -23

# the accuracy csrc/common.h documented when the bounds were set; the bounds stay 1.5 x these (the device's dense-search maxima,
# 4.22e-7 and 3.20e-7, are what the comment there says now)
PAIR_GELU_DOC, PAIR_DGELU_DOC = 4.2e-7, 3.0e-7
B_PAIR_GELU = 1.5 * PAIR_GELU_DOC
B_PAIR_DGELU = 1.5 * PAIR_DGELU_DOC
B_ERF = 2.0 ** -21
BF16_ONLY = 2.0 ** -8

S_CYCLE = (0.0, 1.0, -2.0, 0.5)
SWEEP_M, SWEEP_K, SWEEP_N = 72, 64, 2048
GRID_N, TAIL_N = 1536, 240
GRID_STEP = 12.0 / (GRID_N - 1)
PLANTED = (0.0, -0.0, 1e-30, -1e-30, 4.0, -4.0, 40.0, -40.0, 1e20, -1e20)        # +-4: the clamp of erf_fast
WORST_RECORDED = (3.117, -3.117, 0.083, -0.083)        # where the restatement of gelu_pair_fast is worst (gelu, gelu')


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound over the elements; an element with bound 0 must be exact; a NaN or an infinity counts as inf"""
    got, ref, bound = np.asarray(got, dtype=D), np.asarray(ref, dtype=D), np.asarray(bound, dtype=D)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    if not np.all(np.isfinite(r)):
        return math.inf
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# float64 GELU
# ---------------------------------------------------------------------------------------------------------------------------
def phi64(x):
    """the normal cdf in float64 without cancellation in either tail"""
    x = np.asarray(x, dtype=D)
    t = torch.from_numpy(np.ascontiguousarray(np.abs(x) / math.sqrt(2.0)))
    h = 0.5 * torch.special.erfc(t).numpy()              # the smaller tail, >= 0, exact to float64 rounding
    return np.where(x < 0, h, 1.0 - h)


def gelu64(x):
    x = np.asarray(x, dtype=D)
    return x * phi64(x)


def dgelu64(x):
    x = np.asarray(x, dtype=D)
    return phi64(x) + x * (np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def bound_erf(x):
    return B_ERF * np.maximum(1.0, np.abs(np.asarray(x, dtype=D)))


def sweep_bound(b, scale, ref, bf16_only=False):
    """|got - ref| <= b * scale + 2^-23 |ref| (+ 2^-8 |ref| where only the bf16 output exists)"""
    ref = np.abs(np.asarray(ref, dtype=D))
    return np.asarray(b, dtype=D) * np.asarray(scale, dtype=D) + (ULP + (BF16_ONLY if bf16_only else 0.0)) * ref


# ---------------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------------
def sweep_points():
    """(points fp32 [SWEEP_N], planted bool [SWEEP_N]): a uniform grid on [-6, 6], log-spaced tails out to +-12, the planted points,
    the recorded worst points and seeded uniform points on [-8, 8] for the rest; no infinity, no NaN"""
    grid = np.linspace(-6.0, 6.0, GRID_N)
    tail = np.geomspace(6.0, 12.0, TAIL_N + 1)[1:]
    fixed = np.array(PLANTED + WORST_RECORDED, dtype=D)
    rest = SWEEP_N - (GRID_N + 2 * TAIL_N + fixed.size)
    assert rest >= 0
    rnd = np.random.RandomState(20).uniform(-8.0, 8.0, rest)
    pts = np.concatenate([-tail[::-1], grid, tail, rnd, fixed]).astype(F)
    planted = np.zeros(SWEEP_N, dtype=bool)
    planted[SWEEP_N - fixed.size:] = True
    assert pts.size == SWEEP_N and np.isfinite(pts).all()
    return pts, planted


def sweep_scales(M=SWEEP_M):
    return np.array([S_CYCLE[m % 4] for m in range(M)], dtype=F)


def sweep_A(M=SWEEP_M, K=SWEEP_K):
    """one-hot [M, K]: A[m, m % K] = s_m"""
    A = np.zeros((M, K), dtype=F)
    A[np.arange(M), np.arange(M) % K] = sweep_scales(M)
    return A


def forward_case(M=SWEEP_M):
    """bias [N] carries the sweep: u = fp32(s_m) + fp32(bias[n]) (one fp32 addition), gelu / gelu' of u in float64"""
    pts, _ = sweep_points()
    s = sweep_scales(M)
    u = s[:, None] + pts[None, :]
    assert u.dtype == F
    return dict(bias=pts, s=s, u=u, gelu=gelu64(u), dgelu=dgelu64(u), scale=np.ones_like(u, dtype=D))


def dgrad_case(M=SWEEP_M, bf16=False):
    """aux_in [M, N] carries the sweep, row m shifted by (m / M) of the grid step (planted points stay); with bf16 the points are bf16
    values (returned widened to fp32: the same numbers).  Expected: s_m * gelu'(x) (epilogue 3), s_m * x (epilogue 6)."""
    pts, planted = sweep_points()
    s = sweep_scales(M)
    shift = (np.arange(M, dtype=D) / M * GRID_STEP)[:, None] * (~planted)[None, :]
    x = (pts.astype(D)[None, :] + shift).astype(F)
    x[:, planted] = pts[planted][None, :]                 # (-0.0 + 0.0 would lose its sign)
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
    xd, sd = x.astype(D), s.astype(D)[:, None]
    return dict(aux=x, s=s, dgelu_mul=sd * dgelu64(xd), mul=sd * xd, scale=np.abs(sd) * np.ones_like(xd))


def rne_bf16(x):
    """fp32 numpy -> the bf16 round-to-nearest-even of each value, widened back to fp32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F)).bfloat16().float().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# x3 pieces on the host (round-to-nearest residuals, as tests/test_gemm_x3_gpu.py::test_pieces_are_exact states them)
# ---------------------------------------------------------------------------------------------------------------------------
def split3_host(x):
    """fp32 [rows, cols] -> bf16 [rows, 3, cols]"""
    p1 = x.bfloat16()
    r1 = x - p1.float()
    p2 = r1.bfloat16()
    p3 = (r1 - p2.float()).bfloat16()
    return torch.stack([p1, p2, p3], dim=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the arena
# ---------------------------------------------------------------------------------------------------------------------------
G0 = {4: 4100, 2: 4104}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SENTINEL = {torch.float32: 0xFFC5A5A5 - (1 << 32), torch.bfloat16: 0xFFC5 - (1 << 16)}       # NaNs with a payload, as signed integers
BACK_ROWS = 256


def matrix_index(rows, width, ld):
    return torch.arange(rows)[:, None] * ld + torch.arange(width)[None, :]


def x3_index(rows, cols, row_stride, piece_stride):
    """[rows, 3, cols]: piece p of element (r, c) at r * row_stride + p * piece_stride + c"""
    return torch.arange(rows)[:, None, None] * row_stride + torch.arange(3)[None, :, None] * piece_stride + torch.arange(cols)[None, None, :]


def slab_index(nslab, rows, width, ld, slab_stride):
    return torch.arange(nslab)[:, None, None] * slab_stride + matrix_index(rows, width, ld)[None]


class Arena:
    """flat tensor = front guard | window elements at base + index | back guard.  fill: 'nan' (an input) or 'sentinel' (an output);
    dense = True: no guards at all -- a plain tensor of exactly the window's span (what the existing tests pass)."""

    def __init__(self, index, dtype, device, back, fill, dense=False):
        self.dtype, self.fill = dtype, fill
        isz = torch.empty(0, dtype=dtype).element_size()
        self.g0 = 0 if dense else G0[isz]
        span = int(index.max()) + 1
        total = self.g0 + span + (0 if dense else back)
        self.flat = torch.empty(total, dtype=dtype, device=device)
        if fill == 'nan':
            self.flat.fill_(float('nan'))
        else:
            self.flat.view(INT_VIEW[dtype]).fill_(SENTINEL[dtype])
        self.idx = (index + self.g0).to(device)
        self.inside = torch.zeros(total, dtype=torch.bool, device=device)
        self.inside[self.idx.reshape(-1)] = True
        self.base_bytes = self.g0 * isz
        if not dense and self.flat.is_cuda:
            assert self.ptr % 16 == 0 and self.ptr % 32 == 16, 'the window base must be 16-byte and not 32-byte aligned'

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.base_bytes

    def put(self, x):
        self.flat[self.idx] = x.to(device=self.flat.device, dtype=self.dtype)
        return self

    def get(self):
        return self.flat[self.idx]

    def touched_outside(self):
        """number of elements outside the window that no longer hold the sentinel, and the offset (relative to the window base) of
        the first one"""
        bad = (self.flat.view(INT_VIEW[self.dtype]) != SENTINEL[self.dtype]) & ~self.inside
        n = int(bad.sum())
        return n, (int(torch.nonzero(bad)[0]) - self.g0 if n else None)

    def problems(self, ref=None, tol=None, what='out'):
        """list of contract violations of an OUTPUT arena: stores outside the window, unwritten or NaN elements inside, and (given a
        float64 reference and a tolerance) a result off by tol or more"""
        out = []
        n, first = self.touched_outside()
        if n:
            out.append('%s: %d elements outside the window were written (first at window base %+d)' % (what, n, first))
        got = self.get().double().cpu()
        if torch.isnan(got).any():
            out.append('%s: %d elements of the window are NaN or were not written' % (what, int(torch.isnan(got).sum())))
        elif ref is not None:
            err = (got - ref).abs().max().item()
            if not err < tol:
                out.append('%s: max error %.3g >= %.3g' % (what, err, tol))
        return out


def in_arena(x, pad, device, dense=False, index=None, stride=None):
    """an INPUT: the matrix x [rows, width] at leading dimension width + pad (or at `index`, whose row stride is `stride`), NaN all
    around; the back guard is 257 row strides"""
    rows, width = x.shape[0], x.shape[-1]
    ld = width + pad
    assert index is None or stride is not None, 'an explicit index needs its row stride: the back guard is sized from it'
    idx = matrix_index(rows, width, ld) if index is None else index
    return Arena(idx, x.dtype, device, (BACK_ROWS + 1) * (stride or ld), 'nan', dense).put(x)


def out_arena(rows, width, pad, dtype, device, dense=False, index=None, init=None, stride=None):
    """an OUTPUT window [rows, width] at leading dimension width + pad (or at `index`, whose row stride is `stride`), the sentinel
    everywhere; init: the prior value of an accumulating call"""
    ld = width + pad
    assert index is None or stride is not None, 'an explicit index needs its row stride: the back guard is sized from it'
    idx = matrix_index(rows, width, ld) if index is None else index
    a = Arena(idx, dtype, device, (BACK_ROWS + 1) * (stride or ld), 'sentinel', dense)
    return a.put(init) if init is not None else a
