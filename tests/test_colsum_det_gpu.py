"""GPU: the order-fixed column sums (uniter_colsum_x3_add_det / uniter_colsum_bf16_add_det) give the bits of their numpy restatement
(tests/colsum_det_ref.py), add to `out`, repeat bit for bit, agree with the atomic entry points they replace, and refuse bad
arguments."""
import ctypes

import numpy as np
import pytest
import torch

import colsum_det_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE = -1, -2
# (rows, cols, ld): a ragged last block with few columns, more than one 512-column block with a ragged column tail, exactly one block of
# each, one row
SHAPES = [(197, 8, 16), (197, 520, 528), (64, 512, 512), (1, 8, 8)]


def _case(kind, rows, cols, ld, constructed=False):
    """-> (device operand, prior out, elementwise float32 values [rows, cols], numpy operand for the reference)"""
    if constructed:
        x, out = R.constructed(cols, 3)
        full = x
    else:
        rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols))
        full = (rng.standard_normal((rows, ld)) * 3.0).astype(np.float32)          # the columns beyond `cols` hold values too
        out = rng.standard_normal(cols).astype(np.float32)
    if kind == 'bf16':
        host = R.to_bf16(full)
        dev = torch.from_numpy(host).cuda().to(torch.bfloat16)
        assert torch.equal(dev.float().cpu(), torch.from_numpy(host))
        return dev, out, host[:, :cols], host[:, :cols]
    host = R.split3(full)                                                           # [rows, 3, ld]
    dev = torch.from_numpy(host).cuda().to(torch.bfloat16)
    return dev, out, R.x3_elements(host[:, :, :cols]), host[:, :, :cols]


def _call(kind, dev, rows, cols, ld, out, ws=None, ws_bytes=None, operand=None):
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    need = lib.uniter_colsum_det_ws_bytes(rows, cols)
    if ws is None:
        ws = torch.full((max(need, 4) // 4,), float('nan'), device='cuda')
    fn = lib.uniter_colsum_bf16_add_det if kind == 'bf16' else lib.uniter_colsum_x3_add_det
    return fn(L.ptr(dev) if operand is None else operand, rows, cols, ld, L.ptr(out), L.ptr(ws), need if ws_bytes is None else ws_bytes,
              L.cur_stream())


@pytest.mark.parametrize('kind', ['bf16', 'x3'])
@pytest.mark.parametrize('rows,cols,ld,constructed', [s + (False,) for s in SHAPES] + [(256, 8, 8, True)])
def test_bits_of_the_stated_order(kind, rows, cols, ld, constructed):
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    assert lib.uniter_colsum_det_ws_bytes(rows, cols) == (rows + 63) // 64 * cols * 4
    dev, out0, elems, host = _case(kind, rows, cols, ld, constructed)
    ref1 = (R.colsum_bf16_add_det if kind == 'bf16' else R.colsum_x3_add_det)(host, out0)
    ref2 = (R.colsum_bf16_add_det if kind == 'bf16' else R.colsum_x3_add_det)(host, ref1)
    results = []
    for _ in range(3):
        out = torch.from_numpy(out0).cuda()
        L.check(_call(kind, dev, rows, cols, ld, out), 'colsum_det')
        torch.cuda.synchronize()
        results.append(out.clone())
    # bit-equal to the numpy restatement, and the same bits in three calls
    assert np.array_equal(results[0].cpu().numpy().view(np.uint32), ref1.view(np.uint32))
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    if constructed:
        assert results[0][3].item() == 1.5 and (np.delete(results[0].cpu().numpy(), 3) == 0.5).all()
    # += : a second call adds onto the first one's result
    out = results[0].clone()
    L.check(_call(kind, dev, rows, cols, ld, out), 'colsum_det')
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref2.view(np.uint32))
    # the atomic entry point it replaces computes the same sum in another order: both are within rows * 2^-24 * (|out| + sum |x|) of
    # the exact value (at most `rows` roundings of relative size 2^-24 on any path to the result), so they differ by twice that at most
    atom = torch.from_numpy(out0).cuda()
    if kind == 'bf16':
        L.check(lib.uniter_colsum_bf16_add(L.ptr(dev), rows, cols, ld, L.ptr(atom), L.cur_stream()), 'colsum_bf16_add')
    else:
        L.check(lib.uniter_colsum_x3_add(L.ptr(dev), rows, cols, ld, L.ptr(atom), L.cur_stream()), 'colsum_x3_add')
    torch.cuda.synchronize()
    mag = np.abs(out0).astype(np.float64) + np.abs(elems.astype(np.float64)).sum(0)
    bound = 2 * max(rows, 2) * 2.0 ** -24 * mag
    diff = np.abs(atom.cpu().numpy().astype(np.float64) - results[0].cpu().numpy().astype(np.float64))
    print('%s %s: max |atomic - ordered| / bound = %.3g' % (kind, (rows, cols, ld), float((diff / np.maximum(bound, 1e-300)).max())))
    assert (diff <= bound).all()


@pytest.mark.parametrize('kind', ['bf16', 'x3'])
def test_bad_arguments_are_refused(kind):
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    rows, cols, ld = 130, 16, 16
    dev, out0, _, _ = _case(kind, rows, cols, ld)
    out = torch.from_numpy(out0).cuda()
    need = lib.uniter_colsum_det_ws_bytes(rows, cols)
    assert need == 3 * cols * 4
    ws = torch.zeros(need // 4, device='cuda')

    def refused(rc, code, word):
        assert rc == code, (word, rc)
        assert word.encode() in lib.uniter_last_error(), (word, lib.uniter_last_error())

    refused(_call(kind, dev, rows, cols, ld, out, ws=ws, ws_bytes=need - 4), E_ARG, 'workspace too small')
    refused(_call(kind, dev, rows, cols, ld, out, ws=ws, ws_bytes=0), E_ARG, 'workspace too small')
    refused(_call(kind, dev, rows, cols, ld, out, operand=ctypes.c_void_p(dev.data_ptr() + 2)), E_SHAPE, '16-byte aligned')
    refused(_call(kind, dev, rows, 12, ld, out), E_SHAPE, 'multiples of 8')
    refused(_call(kind, dev, rows, cols, 20, out), E_SHAPE, 'multiples of 8')
    refused(_call(kind, dev, 0, cols, ld, out), E_ARG, 'bad argument')
    refused(_call(kind, dev, rows, cols, 8, out), E_ARG, 'bad argument')            # ld < cols
    fn = lib.uniter_colsum_bf16_add_det if kind == 'bf16' else lib.uniter_colsum_x3_add_det
    refused(fn(L.ptr(dev), rows, cols, ld, L.ptr(out), None, need, L.cur_stream()), E_ARG, 'bad argument')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(out0))                           # nothing was launched
    # and the legal call these vary
    assert _call(kind, dev, rows, cols, ld, out, ws=ws) == 0
    torch.cuda.synchronize()
