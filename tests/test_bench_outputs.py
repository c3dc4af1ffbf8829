"""bench.py --dump-outputs on CPU: what dump_outputs writes for a model's last
step (float32 .npy files, the parameter vectors sampled at fixed indices when
they exceed their share of DUMP_BUDGET), and the plain / --full option
parsing through the SMMD_BENCH_PROBE hook.  No GPU, no library call."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model(n_g, n_d, aux=True):
    g = torch.Generator().manual_seed(3)
    m = types.SimpleNamespace()
    m.last = {'g_loss': torch.tensor(0.25), 'd_loss': torch.tensor(-0.25),
              'aux': torch.arange(8.0) if aux else None}
    m.g_optim = types.SimpleNamespace(flat_param=torch.randn(n_g, generator=g))
    m.d_optim = types.SimpleNamespace(flat_param=torch.randn(n_d, generator=g))
    return m


def test_dump_sample_is_whole_or_a_fixed_sample():
    import bench
    a = np.arange(1000, dtype=np.float64)
    whole = bench.dump_sample(a.reshape(10, 100), 1000)
    assert whole.dtype == np.float32 and np.array_equal(whole, a)
    s1, s2 = bench.dump_sample(a, 100), bench.dump_sample(a + 0.0, 100)
    assert s1.shape == (100,) and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) > 0)                  # sorted, distinct indices
    assert 0 < np.count_nonzero(np.diff(s1) > 1)    # not a leading slice


def test_dump_outputs_writes_the_last_step(tmp_path):
    import bench
    m = _model(300, 500)
    sizes = bench.dump_outputs(m, str(tmp_path / 'o'))
    assert sizes == {'g_loss': 1, 'd_loss': 1, 'aux': 8, 'g_params': 300, 'd_params': 500}
    got = {f[:-4]: np.load(str(tmp_path / 'o' / f)) for f in os.listdir(str(tmp_path / 'o'))}
    assert sorted(got) == sorted(sizes) and all(a.dtype == np.float32 for a in got.values())
    assert float(got['g_loss']) == 0.25 and float(got['d_loss']) == -0.25
    assert np.array_equal(got['aux'], np.arange(8, dtype=np.float32))
    assert np.array_equal(got['g_params'], m.g_optim.flat_param.numpy())
    assert np.array_equal(got['d_params'], m.d_optim.flat_param.numpy())


def test_dump_outputs_stays_within_the_budget(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_BUDGET <= 64 * 1000 * 1000
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 4000)         # 1000 floats in all
    m = _model(300, 5000, aux=False)
    sizes = bench.dump_outputs(m, str(tmp_path))
    assert sizes == {'g_loss': 1, 'd_loss': 1, 'g_params': 300, 'd_params': 499}
    assert sum(sizes.values()) * 4 <= 4000
    again = bench.dump_outputs(m, str(tmp_path / 'again'))
    assert again == sizes
    a, b = np.load(str(tmp_path / 'd_params.npy')), np.load(str(tmp_path / 'again' / 'd_params.npy'))
    assert np.array_equal(a, b) and np.isin(a, m.d_optim.flat_param.numpy()).all()


PLAIN = ['--gpus', '1', '--steps', '5', '--warmup', '2']
EXTRAS = ('ref_schedule', 'instrumented', 'step_flops', 'mmd_sweep', 'cpu_baseline')


def test_plain_run_skips_every_other_measurement():
    import bench
    for argv in (PLAIN, [], PLAIN + ['--instrument-cycles', '1', '--mmd-sweep', '2',
                                      '--ref-schedule-steps', '6', '--cpu-steps', '3']):
        p = bench.run_parts(bench.parse_args(argv))
        assert p['prime_schedules'] == ('lean',)
        assert not any(p[k] for k in EXTRAS), p
        assert p['dump_outputs'] is False
    p = bench.run_parts(bench.parse_args(PLAIN + ['--dump-outputs', 'd']))
    assert p['dump_outputs'] is True and not any(p[k] for k in EXTRAS)
    assert bench.parse_args(PLAIN).steps == 5 and bench.parse_args(PLAIN).warmup == 2


def test_full_enables_them_under_their_own_options():
    import bench
    p = bench.run_parts(bench.parse_args(PLAIN + ['--full']))
    assert p['prime_schedules'] == ('lean', 'reference')
    assert all(p[k] for k in EXTRAS), p
    off = {'ref_schedule': ['--ref-schedule-steps', '0'],
           'instrumented': ['--instrument-cycles', '0'],
           'mmd_sweep': ['--mmd-sweep', '0'], 'cpu_baseline': ['--no-cpu-baseline']}
    for part, argv in off.items():
        p = bench.run_parts(bench.parse_args(PLAIN + ['--full'] + argv))
        assert not p[part] and all(p[k] for k in EXTRAS if k != part), (part, p)
    # the CPU baseline: rank 0 of a one-GPU run only; the dump: rank 0 only
    a = bench.parse_args(['--gpus', '2', '--full', '--dump-outputs', 'd'])
    assert not bench.run_parts(a, world=2, rank=0)['cpu_baseline']
    assert bench.run_parts(a, world=2, rank=0)['dump_outputs']
    assert not bench.run_parts(a, world=2, rank=1)['dump_outputs']


def test_full_and_dump_outputs_are_options():
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['SMMD_BENCH_PROBE'] = '1'
    for extra in ([], ['--full'], ['--full', '--dump-outputs', 'unused']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                            '--steps', '2', '--warmup', '1'] + extra,
                           capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert '"probe": true' in r.stdout
