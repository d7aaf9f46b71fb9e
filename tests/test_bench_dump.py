"""bench.py --dump-outputs: what the headline run's last timed step returned, written as float32 .npy files (CPU: the writer and the
argument checks; -m gpu: one small bench run end to end)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench


def test_dump_writes_float32_arrays_whole_when_small(tmp_path):
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(8, 71, generator=g).to(torch.bfloat16)
    loss = torch.tensor([0.6931], dtype=torch.float32)
    written = bench.dump_outputs(str(tmp_path / 'd'), {'loss': loss, 'logits': logits})
    assert written == {'loss': [1], 'logits': [8, 71]}
    assert sorted(os.listdir(tmp_path / 'd')) == ['logits.npy', 'loss.npy']
    a = np.load(tmp_path / 'd' / 'logits.npy')
    assert a.dtype == np.float32 and np.array_equal(a, logits.float().numpy())
    assert np.load(tmp_path / 'd' / 'loss.npy').dtype == np.float32


def test_dump_samples_large_arrays_the_same_way_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 1000)
    t = torch.arange(50_000, dtype=torch.float64).reshape(50, 1000)
    bench.dump_outputs(str(tmp_path / 'a'), {'params': t})
    bench.dump_outputs(str(tmp_path / 'b'), {'params': t.clone()})
    a, b = np.load(tmp_path / 'a' / 'params.npy'), np.load(tmp_path / 'b' / 'params.npy')
    assert a.dtype == np.float32 and 900 < a.size <= 1000
    assert np.array_equal(a, b)                                   # a fixed sample: the same elements on every run
    assert np.all(np.diff(a) > 0) and np.all(a == np.round(a))    # distinct elements of the array, in index order


def test_dump_refuses_more_than_its_byte_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4 * 100)
    with pytest.raises(RuntimeError, match='dump-outputs'):
        bench.dump_outputs(str(tmp_path), {'a': torch.zeros(60), 'b': torch.zeros(60)})


def test_steps_must_be_positive():
    assert bench.parse_args(['--steps', '3', '--warmup', '0']).steps == 3
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


@pytest.mark.gpu
def test_bench_dump_outputs_end_to_end(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    d = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'tiny2', '--batch', '8', '--length', '1000',
                        '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--dump-outputs', str(d)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['steps'] == 3
    assert out['dumped_outputs']['arrays'] == {'loss': [1], 'logits': [8, 71], 'grad_norm': [1], 'params': [out['dumped_outputs']['arrays']['params'][0]]}
    arrays = {n: np.load(d / f'{n}.npy') for n in ('loss', 'logits', 'grad_norm', 'params')}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays['loss'][0]) == pytest.approx(out['final_loss'], rel=1e-6)   # the last timed step's loss
    assert arrays['grad_norm'][0] > 0
