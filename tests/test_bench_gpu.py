"""GPU: bench.py keeps its output contract (one JSON line with the driver's keys; with --full also the roofline and
cpu_baseline objects), a plain run's --dump-outputs does not depend on the clock warm-up, and __graft_entry__.smoke() runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', *flags],
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_default_contract():
    d = _bench('--full')
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['unit'] == 'samples/s' and d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1
    assert d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['dtype'] == 'f32' and d['data'] == 'synthetic' and 'workload' in d['config'] and 'model' not in d['config']
    assert abs(d['value'] - 16 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-3
    # the default is the fp32 step with its dense products as six bf16 MFMA products per block (three bf16 pieces per value):
    # dtype f32, the workload says so, the roofline prices the products on the bf16 pipe / 6 and the SAME process times the
    # native fp32 MFMA kernels next to it
    assert '3 x bf16' in d['config']['workload'] and '6 MFMA products' in d['config']['workload']
    r = d['roofline']
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and abs(r['peak'] - 2500.0 / 6) < 0.1
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and 0.1 < r['frac'] < 1.0
    assert d['peak_tflops']['dense_products'] == 416.7 and d['peak_tflops']['attention'] == 416.7      # L = 164: the attention's products are x3 products too
    nat = d['native_fp32']
    assert nat['value'] > 0 and abs(nat['value'] - 16 / (nat['ms_per_step'] * 1e-3)) / nat['value'] < 1e-3
    assert d['value'] > nat['value']                   # the point of the mode
    # the GEMM family that takes the most time of the step, stamped inside the timed region; every family is listed
    fams = {f['family']: f for f in d['roofline_families']}
    assert {'gemm_ffn_up_fwd', 'gemm_ffn_down_fwd', 'gemm_qkv_fwd', 'gemm_attn_out_fwd', 'gemm_dgrad', 'gemm_wgrad',
            'attention_fwd', 'attention_bwd', 'layernorm_fwd', 'layernorm_bwd'} <= set(fams)
    assert fams['gemm_ffn_up_fwd']['launches_per_step'] == 12 and fams['gemm_dgrad']['launches_per_step'] == 48
    assert all('in-kernel stamps' in f['measured'] for n, f in fams.items() if n.startswith('gemm_'))
    assert r['kernel'].split(':')[0] in fams and r['launches'] == 3 * fams[r['kernel'].split(':')[0]]['launches_per_step']
    for f in fams.values():
        assert 0.0 < f['frac'] < 1.0, f
    assert d['optimizer']['bound'] == 'hbm' and 0.05 < d['optimizer']['frac'] < 1.0
    # both gradient GEMM families over the time either of them ran: above each family's own in-situ rate, below the peak
    t = d['backward_gemms_together']
    dg, wg = fams['gemm_dgrad'], fams['gemm_wgrad']
    assert min(dg['frac'], wg['frac']) < t['frac'] < 1.0
    # The invariant of the two backward streams: the union of both families' launch intervals is shorter than their sum (they DO
    # run beside each other) and no shorter than the longer family.  (The stronger `max(frac) < together` of round 3 is a property
    # of the native fp32 mode, whose 64-KB workgroups share CUs: in the fp32x3 mode two persistent 144-KB workgroups cannot, the
    # streams time-slice at workgroup granularity, and a family stamped from its first workgroup's start to its last one's end
    # contains the other one's slices -- its own fraction can then exceed the union's by a hair.  ADVICE r04.)
    assert max(dg['ms_per_step'], wg['ms_per_step']) - 1e-6 <= t['ms_per_step'] <= 0.98 * (dg['ms_per_step'] + wg['ms_per_step'])
    assert t['frac'] > 0.9 * max(dg['frac'], wg['frac'])
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['unit'] == 'samples/s' and c['value'] > 0 and c['cores'] >= 1 and c['sample']
    assert c['single_thread']['value'] > 0 and c['gflops'] > 0 and c['cpu_model'] and c['os_cpu_count'] >= c['cores']
    # N = the physical cores the process may use, and 32 threads where that differs: both in the block, `cores` = the one reported
    assert c['physical_cores'] >= 1 and c['by_cores'][0]['cores'] == c['physical_cores']
    ran = [l for l in c['by_cores'] if l['steps'] > 0]
    assert ran and c['cores'] in [l['cores'] for l in ran] and c['value'] == max(l['value'] for l in ran)
    assert all(l['steps'] > 0 or ('note' in l and l['cores'] > 64) for l in c['by_cores'])      # an all-cores leg that did not run says so
    # the same step in the bf16 mode (BASELINE configs[2] arithmetic), same process: a driver-timed bf16 figure
    b16 = d['bf16']
    assert b16['dtype'] == 'bf16' and b16['value'] > d['value'] and abs(b16['value'] - 16 / (b16['ms_per_step'] * 1e-3)) / b16['value'] < 1e-3
    assert 0.02 < b16['step_mfma_frac'] < 1.0 and b16['peak_tflops'] == 2500.0 and b16['final_loss'] == b16['final_loss']
    # both durations of the dominant family: in-kernel stamps (frac) and HIP events with the queueing included (frac_dispatch)
    assert r['avg_ms'] > 0 and r['avg_ms_dispatch'] > 0 and 0.0 < r['frac_dispatch'] < 1.0 and 'stamps' in r['note']
    # round 6: the bound that applies, per family -- recomputed here from the shape for one family: FFN-up forward
    # at configs[1] is M = 2624, N = 3072, K = 768 on 128 x 256 x3 tiles (252 work items, three pieces: 72 KB staged per k-tile)
    fl = fams['gemm_ffn_up_fwd']['floor']
    M, N, K = 2624, 3072, 768
    mfma = 2.0 * M * N * K / (2500e12 / 6) * 1e6
    staged = 21 * 12 * (K // 32) * (128 + 256) * 32 * 2 * 3
    intake = staged / (70e9 * 252) * 1e6
    hbm = (M * K * 6 + N * K * 6 + M * N * 10) / 8e12 * 1e6
    assert abs(fl['mfma_us'] - mfma) < 0.02 and abs(fl['intake_us'] - intake) < 0.02 and abs(fl['hbm_us'] - hbm) < 0.02
    assert abs(fl['floor_us'] - max(mfma, intake, hbm)) < 0.02 and fl['launches'][0]['tile'] == '128x256' and fl['launches'][0]['items'] == 252
    f_up = fams['gemm_ffn_up_fwd']
    assert abs(f_up['floor_ms_per_step'] - 12 * fl['floor_us'] * 1e-3) < 1e-3 and abs(f_up['over_floor'] - f_up['ms_per_step'] / f_up['floor_ms_per_step']) < 0.01
    assert all(f.get('over_floor', 2.0) > 1.0 for f in fams.values())                    # nothing runs below its floor
    assert abs(d['step_floor_ms'] - sum(f['floor_ms_per_step'] for f in fams.values())) < 1e-2 and d['step_over_floor'] > 1.0
    assert 'attn_x3' in d['attention_kernel']
    # the short figures close the line: the last key is the summary, and it repeats them
    assert list(d)[-1] == 'summary' and list(d).index('roofline_families') < list(d).index('roofline') < list(d).index('bf16')
    sm = d['summary']
    assert sm['value'] == d['value'] and sm['bf16']['value'] == b16['value'] and sm['native_fp32']['value'] == nat['value']
    assert sm['over_floor']['gemm_ffn_up_fwd'] == f_up['over_floor'] and sm['roofline']['frac'] == r['frac'] and sm['cpu_baseline']['cores'] == c['cores']
    assert len(json.dumps(sm)) < 2000


def test_bench_native_fp32_mode_keeps_its_roofline():
    d = _bench('--full', '--precision', 'fp32', '--no_cpu_baseline')
    assert d['dtype'] == 'f32' and d['roofline']['peak'] == 157.3 and 'native fp32 MFMA' in d['config']['workload']
    assert 'native_fp32' not in d and d['peak_tflops']['dense_products'] == 157.3 and d['peak_tflops']['attention'] == 157.3


@pytest.mark.parametrize('flags', [('--precision', 'bf16', '--no_cpu_baseline'),
                                   ('--ragged', '--packed', '--no_cpu_baseline'),
                                   ('--workload', 'multitask', '--batch', '8', '--no_cpu_baseline')])
def test_bench_variants_run(flags):
    d = _bench('--full', *flags)
    assert d['value'] > 0 and 'cpu_baseline' not in d


@pytest.mark.parametrize('extra', [(), ('--dp_sparse_embeddings',), ('--precision', 'bf16', '--dp_sparse_embeddings')])
def test_bench_starts_its_own_ranks(extra):
    """`python bench.py --gpus 2` with no launcher environment (the shape of the driver's command): the process starts two
    fresh ranks itself and the line reports what torch.distributed saw.  Two ranks on ONE GPU: gloo (RCCL wants one device
    per rank) -- the launcher, the rendezvous, the exchange and the line are the ones an 8-GPU run uses."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    env.update(UNITER_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--full', '--gpus', '2', '--steps', '2', '--warmup', '1',
                          '--prewarm_s', '0', '--prof_kind', '0', '--no_cpu_baseline', *(extra or ()), *(('--no_reserve_pick',) if extra else ())],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['ranks_seen'] == 2 and d['config']['dist_backend'] == 'gloo'
    assert d['config']['global_batch'] == 32 and d['config']['parallelism'] == 'dp2' and 'self-spawned' in d['config']['launcher']
    # (gloo moves 440 MB of gradients through the host: seconds per step -- the value is rounded to two decimals)
    assert abs(d['value'] - 32 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-2 and d['final_loss'] == d['final_loss']
    n_sparse = d['config']['dp_sparse_embedding_steps']            # every step took the sparse path (warm-up and the events pass included)
    assert (n_sparse == 0) if not extra else (n_sparse == 2 + 1)
    # the exchange explains itself: payload, bytes and timing of every collective of a step, what the optimizer waited for
    c = d['comm']
    assert c['world'] == 2 and c['payload'] == ('bf16' if 'bf16' in extra else 'fp32') and c['sparse_embeddings'] == bool('--dp_sparse_embeddings' in extra)
    assert c['collectives'] and all(k['bytes'] > 0 and k['issue_to_done_ms'] >= k['exposed_ms'] >= 0 for k in c['collectives'])
    assert c['bytes_per_step'] > 0 and c['exposed_ms_per_step'] >= 0 and c['headline_exchange'] in ('dense', 'sparse word-embedding rows')
    assert c['rccl_max_nchannels_env'] is None                 # RCCL's channel count is RCCL's (UNITER_DP_CAP_CHANNELS=1 caps it at the reserve)
    if extra:
        assert c['cu_reserve'] == 16 and 'reserve_pick' not in c           # two ranks: the persistent launches leave 16 CUs
    else:
        # the default: a few untimed steps with the reserve and without it, the faster kept on every rank (dp.pick_cu_reserve)
        rp = c['reserve_pick']
        assert [k['cu_reserve'] for k in rp['candidates']] == [16, 0, 48] and all(k['ms_per_step'] > 0 for k in rp['candidates'])
        assert rp['picked'] in (16, 0, 48) and c['cu_reserve'] == rp['picked']


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run carries the headline only; --dump-outputs writes the last timed step's loss, probabilities and a sample of the
    updated parameters and Adam moments.  The clock warm-up (a time, not a step count) runs on a throwaway copy of the model: with
    and without it the timed steps start from the same state and compute the same outputs, up to the order of float atomics."""
    runs = []
    for tag, extra in (('warm', ()), ('cold', ('--prewarm_s', '0'))):
        d = _bench('--dump-outputs', str(tmp_path / tag), *extra)
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in d, k
        assert d['steps'] == 3 and d['dtype'] == 'f32' and d['higher_is_better'] is True and d['unit'] == 'samples/s'
        assert abs(d['value'] - 16 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-3
        for k in ('roofline', 'roofline_families', 'native_fp32', 'bf16', 'optimizer', 'cpu_baseline'):
            assert k not in d, k
        files = sorted(os.listdir(str(tmp_path / tag)))
        assert files == ['adam_exp_avg_sample.npy', 'adam_exp_avg_sq_sample.npy', 'loss.npy', 'params_sample.npy', 'probs.npy']
        arr = {f[:-4]: np.load(str(tmp_path / tag / f)) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arr.values())
        assert sum(a.nbytes for a in arr.values()) <= 64 << 20
        assert arr['probs'].shape == (16,) and arr['params_sample'].shape == (1 << 22,) and abs(arr['loss'][0] - d['final_loss']) < 1e-4
        runs.append(arr)
    a, b = runs
    assert abs(a['loss'][0] - b['loss'][0]) <= 1e-5 * abs(a['loss'][0]) and np.abs(a['probs'] - b['probs']).max() <= 1e-5
    # (a warm-up on the timed model itself would be ~100 more Adam steps: parameters 1e-4 .. 1e-3 away)
    assert np.abs(a['params_sample'] - b['params_sample']).max() <= 1e-6
    for k in ('adam_exp_avg_sample', 'adam_exp_avg_sq_sample'):
        assert np.abs(a[k] - b[k]).max() <= 1e-3 * np.abs(a[k]).max()


def test_graft_entry_smoke():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.smoke()
