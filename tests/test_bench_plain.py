"""bench.py without --full does the headline leg alone: no roofline step, no other arithmetic modes, no inference legs, no CPU baseline.
CPU tier: which parts each command line turns on.  GPU tier: a plain run's result line holds the headline and none of the extras."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ('no_roofline', 'no_extra_modes', 'no_inference', 'no_d4', 'no_cpu_baseline')


def test_plain_run_turns_every_extra_off():
    a = bench.parse(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not a.full and all(getattr(a, k) for k in EXTRAS)


def test_full_run_keeps_every_extra_unless_switched_off():
    a = bench.parse(['--full'])
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = bench.parse(['--full', '--no-d4', '--no-cpu-baseline'])
    assert a.no_d4 and a.no_cpu_baseline and not (a.no_roofline or a.no_extra_modes or a.no_inference)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_only():
    args = ['--gpus', '1', '--batch', '2', '--size', '128', '--steps', '2', '--warmup', '1']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = lines[0]
    assert out['metric'] == 'images/sec EfficientDet-D0 512px fwd+bwd' and out['unit'] == 'images/sec' and out['higher_is_better'] is True
    assert out['value'] > 0 and out['ms_per_step'] > 0 and out['steps'] == 2 and out['dtype'] == 'f32_hf16x3_bwd_bf16x3'
    for k in ('roofline', 'inference', 'inference_d4', 'cpu_baseline') + tuple(bench.EXTRA_KEY.values()):
        assert k not in out, k
