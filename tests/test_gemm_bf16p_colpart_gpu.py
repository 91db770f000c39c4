"""GPU: the column-partial epilogue of the persistent bf16 kernel (csrc/gemm_bf16_p.hip: P1_MUL with g.colpart) through its own C-ABI
entry, uniter_gemm_bf16p_colpart -- dU = (A . W) * aux stored as bf16 on 128 x 256 tiles and, per 64 output rows, one row of N fp32
column sums of the STORED values.  Inside the model it runs only under UNITER_B16_PERSIST bits 4 + 8 (model.cpp: linear() with a
colpart pointer); here it is held to float64 on the arenas of tests/gemm_ref.py.

Layout.  A [M, K], W [K, N] (k-major: the input-gradient layout) and aux [M, N] each sit at a leading dimension 8 elements wider than
the matrix, at a base that is 16-byte and not 32-byte aligned, NaN all around -- the padding columns, the rows right behind row M - 1,
both guards: a kernel that took "rows beyond M hold zeros" from memory instead of from its buffer ranges would sum a NaN into the
partial row of a ragged last block.  The bf16 output sits in a sentinel arena at a padded leading dimension; the partials in a
sentinel arena of exactly ceil(M / 64) rows of N floats whose back guard (256 rows) covers every row a 128-row tile could reach: the
model allocates (M + 31) / 32 rows and reads (M + 63) / 64, so a row whose 64 output rows lie wholly beyond M must stay untouched.

Operands.  The accumulator is exact in fp32 for every summation order, as in gemm_ref.py's sweep: A is one-hot, A[m, m % K] = s_m with
s_m cycling over (0, 1, -2, 0.5), and W holds signed powers of two that depend on (k, n), so acc[m, n] = s_m * W[m % K, n] exactly and
a wrong k-row or column of W shows.  aux is seeded normal (fp32, or bf16 values for the bf16 aux).

Checks, per shape:
  1. the bf16 output against s_m * W[m % K, n] * aux[m, n] in float64 at gemm_ref.py's bound of epilogue 6 for a bf16-only output:
     B = 0, i.e. (2^-23 + 2^-8) |ref| -- one fp32 product rounding and the bf16 store;
  2. the bf16 output bit-identical to uniter_gemm_bf16v2_cfg(7, ...) on the same arenas without the partials;
  3. every partial row i against the float64 sum of rows 64 i .. 64 i + 63 of the kernel's OWN stored output.  Each stored value is
     exact in fp32, and a partial is an fp32 sum of at most 64 of them in some order: at most 63 additions, each rounding a partial
     sum of magnitude <= sum |v| by <= 2^-24 of it, so |partial - exact| <= 64 * 2^-24 * sum_{rows of the block} |v| per column;
     summed over the ceil(M / 64) rows the same bound with the sum over all rows (asserted as well).  Derived, not measured.
Shapes: M in {1, 63, 64, 65, 128, 129, 228, 257} (one row; one wave short of, at and past its 64 rows; one tile, one row past it; the
model's 228; two tiles and one row) x N in {256, 264, 2048} (one tile wide; 8 columns into a second tile; eight tiles) x K in
{64, 192} (one k-tile: shorter than the loaders' two-tile lead; three) x aux in fp32 and bf16.

b_kmajor: the x aux epilogue of the persistent kernels is built for k-major weights only (gemm_b1p_run: "epilogue 6 is not built for
k-contiguous weights"), so 1 is the one value the entry accepts; 0 must fail with an argument error and write nothing.

Measured on an MI355X over all 96 shapes: the partial rows and their sum over the rows reach at most 0.013 of the derived bound 3;
the bf16 output 0.996 of bound 1 with the fp32 aux (the bf16 store's own half ulp) and is exact with the bf16 aux (a product of two
8-bit significands by a power of two fits bf16).  No store outside either window, no partial row beyond ceil(M / 64), no NaN taken from
behind row M: the epilogue's "rows beyond M hold zeros" holds because the operand and aux buffer ranges end at row M, whatever the
leading dimension.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
PAD = 8
MS = [1, 63, 64, 65, 128, 129, 228, 257]
NS = [256, 264, 2048]
KS = [64, 192]
W_CYCLE = (1.0, -2.0, 0.5, 4.0, -1.0)        # signed powers of two: s_m * w is exact in fp32 (and in bf16)
SHARES = {'out': 0.0, 'part': 0.0}


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def _weights(K, N):
    k, n = torch.arange(K)[:, None], torch.arange(N)[None, :]
    return torch.tensor(W_CYCLE)[(3 * k + n + n // 16) % len(W_CYCLE)]


def _run(M, N, K, aux_bf16, bkm=1):
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    s = R.sweep_scales(M)
    A = torch.from_numpy(R.sweep_A(M, K))
    W = _weights(K, N)
    g = torch.Generator().manual_seed(1000 * M + N + K)
    aux = torch.randn(M, N, generator=g)
    if aux_bf16:
        aux = aux.bfloat16().float()
    a = R.in_arena(A.bfloat16(), PAD, DEV)
    b = R.in_arena(W.bfloat16() if bkm else W.t().contiguous().bfloat16(), PAD, DEV)
    x = R.in_arena(aux.bfloat16() if aux_bf16 else aux, PAD, DEV)
    nrows = (M + 63) // 64
    outs = []
    for with_part in (True, False):
        Cb = R.out_arena(M, N, PAD, BF, DEV)
        part = R.out_arena(nrows, N, 0, F32, DEV) if with_part else None
        ldb = (N if bkm else K) + PAD
        if with_part:
            rc = lib.uniter_gemm_bf16p_colpart(bkm, M, N, K, _vp(a), K + PAD, _vp(b), ldb, None, 0, _vp(Cb), N + PAD, _vp(x),
                                               int(aux_bf16), N + PAD, _vp(part), L.cur_stream())
        else:
            rc = lib.uniter_gemm_bf16v2_cfg(7, 1, 0, bkm, M, N, K, _vp(a), K + PAD, _vp(b), ldb, None, 0, 0, _vp(Cb), N + PAD, 6, None,
                                            _vp(x), int(aux_bf16), None, 0, N + PAD, 0, L.cur_stream())
        torch.cuda.synchronize()
        outs.append((rc, Cb, part))
        if not bkm:
            break
    ref = s.astype(np.float64)[:, None] * W[torch.arange(M) % K].double().numpy() * aux.double().numpy()
    return outs, ref


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_column_partials_of_the_stored_bf16_output(M, N):
    from meme_challenge_amd import _lib as L
    nrows = (M + 63) // 64
    for K in KS:
        for aux_bf16 in (False, True):
            tag = (M, N, K, aux_bf16)
            ((rc, Cb, part), (rc2, Cb2, _)), ref = _run(M, N, K, aux_bf16)
            L.check(rc, 'gemm_bf16p_colpart')
            L.check(rc2, 'gemm_bf16v2_cfg')
            # nothing outside either window, every element inside written -- the partial rows at ceil(M / 64) and beyond included
            bad = Cb.problems(what='C_bf16') + part.problems(what='colpart') + Cb2.problems(what='C_bf16 (no partials)')
            assert not bad, tag + tuple(bad)
            # 1. the product against float64
            got = Cb.get().float().cpu().numpy()
            r1 = R.worst_ratio(got, ref, R.sweep_bound(0.0, 1.0, ref, bf16_only=True))
            SHARES['out'] = max(SHARES['out'], r1)
            # 2. the same bits as the product without the partials
            same = torch.equal(Cb.get().view(torch.int16), Cb2.get().view(torch.int16))
            # 3. the partials against the float64 column sums of the stored output
            v = got.astype(np.float64)
            p = part.get().cpu().numpy().astype(np.float64)
            r3 = 0.0
            for i in range(nrows):
                blk = v[64 * i:64 * i + 64]
                r3 = max(r3, R.worst_ratio(p[i], blk.sum(0), 64 * 2.0 ** -24 * np.abs(blk).sum(0)))
            r3s = R.worst_ratio(p.sum(0), v.sum(0), 64 * 2.0 ** -24 * np.abs(v).sum(0))
            SHARES['part'] = max(SHARES['part'], r3, r3s)
            print('colpart M=%d N=%d K=%d aux_bf16=%d: output %.3g of its bound, partial rows %.3g, their sum %.3g of the derived bound; '
                  'worst so far %.3g / %.3g' % (M, N, K, aux_bf16, r1, r3, r3s, SHARES['out'], SHARES['part']))
            assert r1 <= 1.0, tag + ('output', r1)
            assert same, tag + ('the partials changed the stored product',)
            assert r3 <= 1.0 and r3s <= 1.0, tag + ('partials', r3, r3s)
            assert np.abs(v).sum() > 0 or M == 1          # (row 0 has s_0 = 0: M = 1 is the all-zero product, partials exactly 0)


def test_k_contiguous_weights_are_refused_without_a_store():
    """b_kmajor = 0: the x aux epilogue is not built for k-contiguous weights -- an argument error, no launch, both outputs untouched"""
    ((rc, Cb, part),), _ = _run(129, 264, 64, False, bkm=0)
    assert rc != 0
    assert Cb.touched_outside()[0] == 0 and part.touched_outside()[0] == 0
    assert bool(torch.isnan(Cb.get().float()).all()) and bool(torch.isnan(part.get()).all())
