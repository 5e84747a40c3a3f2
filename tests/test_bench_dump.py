"""bench.py --dump-outputs: what the headline's last timed step computed, written as DIR/<name>.npy so that two builds can be compared
output for output.  CPU tier: the writer (dtype, 64 MB cap, fixed sample) and the argument checks.  GPU tier: two runs with the same
arguments write identical arrays, and --steps is the number of timed steps the result line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_float32_whole_when_it_fits(tmp_path):
    out = {'a': torch.arange(10, dtype=torch.bfloat16), 'b': torch.ones(3, dtype=torch.float64), 'c': np.arange(5, dtype=np.int64)}
    assert bench.dump_outputs(str(tmp_path), out) == ['a', 'b', 'c']
    a, b, c = (np.load(tmp_path / (k + '.npy')) for k in 'abc')
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(10, dtype=np.float32))
    assert b.dtype == np.float64 and np.array_equal(b, np.ones(3))
    assert c.dtype == np.float32 and np.array_equal(c, np.arange(5, dtype=np.float32))


def test_dump_directory_it_creates_is_git_ignored(tmp_path):
    d = tmp_path / 'new'
    bench.dump_outputs(str(d), {'x': torch.zeros(2)})
    assert (d / '.gitignore').read_text() == '*\n'
    bench.dump_outputs(str(tmp_path), {'x': torch.zeros(2)})                  # an existing directory is left as it is
    assert not (tmp_path / '.gitignore').exists()


def test_dump_cuts_large_outputs_to_a_fixed_sample_within_the_cap(tmp_path):
    budget = 1 << 20
    big = torch.arange(1 << 20, dtype=torch.float32)                          # 4 MB: 4x the cap on its own
    small = torch.tensor([1.5, 2.5])
    for d in ('r1', 'r2'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small}, budget=budget)
        assert _files_bytes(tmp_path / d) <= budget
    s1, s2 = np.load(tmp_path / 'r1' / 'big.npy'), np.load(tmp_path / 'r2' / 'big.npy')
    assert np.array_equal(s1, s2)                                             # the same sample on every run
    assert s1.size > (budget // 4) // 2 and np.all(np.diff(s1) > 0)           # most of the cap used; sorted distinct elements of `big`
    assert np.array_equal(np.load(tmp_path / 'r1' / 'small.npy'), small.numpy())


def test_dump_default_cap_is_64_mb():
    assert bench.DUMP_BUDGET_BYTES <= 64 * 1000 * 1000


def test_steps_must_be_at_least_one():
    for argv in (['--steps', '0'], ['--extra-steps', '0']):
        with pytest.raises(SystemExit):
            bench.parse(argv)
    a = bench.parse(['--steps', '7', '--dump-outputs', 'rel_dir'])
    assert a.steps == 7 and os.path.isabs(a.dump_outputs)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_outputs_are_reproducible_and_steps_are_timed(tmp_path):
    args = ['--gpus', '1', '--batch', '2', '--size', '128', '--steps', '3', '--warmup', '1',
            '--no-roofline', '--no-extra-modes', '--no-inference', '--no-cpu-baseline']
    dirs = []
    for i in range(2):
        d = str(tmp_path / ('run%d' % i))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args + ['--dump-outputs', d],
                           capture_output=True, text=True, timeout=800, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1 and lines[0]['steps'] == 3, r.stdout[-2000:]
        assert sorted(f for f in os.listdir(d) if f.endswith('.npy')) == ['cls_loss.npy', 'parameters.npy', 'reg_loss.npy']
        assert _files_bytes(d) <= bench.DUMP_BUDGET_BYTES
        dirs.append(d)
    for name in ('cls_loss', 'reg_loss', 'parameters'):
        x, y = (np.load(os.path.join(d, name + '.npy')) for d in dirs)
        assert x.dtype == np.float32 and np.all(np.isfinite(x)), name
        assert np.array_equal(x, y), name                                     # the path has no float atomics: bit for bit
    assert np.load(os.path.join(dirs[0], 'parameters.npy')).size > 1000000
