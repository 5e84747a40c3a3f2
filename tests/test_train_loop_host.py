"""CPU tier of the captured training loop (train.py:104-120 as device gates): the additive entry points of csrc/optim.hip are declared,
exported and refuse bad arguments before they launch anything; the Python surface exists and refuses what it must; the documents name
the class.  Builds and loads the library; no GPU call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('effdet_train_gate', 'effdet_grad_accumulate', 'effdet_clip_adamw_step_gated')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.require(*NEW)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_abi_generation_stays(lib):
    from efficientdet.pytorch_amd import _lib
    h = _header()
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, h), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert 'effdet_train_ctl_t' in h
    assert int(re.search(r'#define\s+EFFDET_ABI_VERSION\s+(\d+)', h).group(1)) == 11
    assert int(lib.effdet_abi_version()) == 11 == _lib.ABI_VERSION
    # the old entry point keeps its signature: 20 parameters, write_grad and hyper_dev in front of the stream
    old = re.search(r'int\s+effdet_clip_adamw_step\s*\((.*?)\)\s*;', h, flags=re.S).group(1)
    assert len(old.split(',')) == 20 and 'int write_grad, const float* hyper_dev, effdet_stream_t stream' in ' '.join(old.split())


def test_control_block_layout_matches_the_header_as_gcc_sees_it(tmp_path):
    import shutil
    import subprocess
    from efficientdet.pytorch_amd import _lib
    fields = [n for n, _ in _lib.TrainCtl._fields_]
    assert fields == ['skip', 'pending', 'applied', 'skipped', 'loss_count', 'loss_sum'] and C.sizeof(_lib.TrainCtl) == 32
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'ctl.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_hip.h"\nint main(void){printf("%zu\\n", sizeof(effdet_train_ctl_t));'
                   + ''.join('printf("%%zu\\n", offsetof(effdet_train_ctl_t, %s));' % f for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'ctl'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.TrainCtl)
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.TrainCtl, f).offset == off, f


P = C.c_void_p(0x1000)         # "some non-null pointer": never dereferenced, every call below is refused before a launch
N = C.c_void_p(0)


def test_gate_refuses_null_arguments(lib):
    assert lib.effdet_train_gate(N, P, N) == EINVAL
    assert lib.effdet_train_gate(P, N, N) == EINVAL


def test_accumulate_refuses_null_tables_and_empty_grids(lib):
    good = [P, P, P, P, P, 1, 1, P, N]          # grads, acc, numel, block_tensor, block_first, ntensors, nblocks, ctl, stream
    for i in (0, 1, 2, 3, 4, 7):
        a = list(good); a[i] = N
        assert lib.effdet_grad_accumulate(*a) == EINVAL, i
    for i in (5, 6):
        for bad in (0, -3):
            a = list(good); a[i] = bad
            assert lib.effdet_grad_accumulate(*a) == EINVAL, (i, bad)


def test_gated_step_refuses_null_tables_and_empty_grids(lib):
    f = C.c_float
    # params, grads, acc, exp_avg, exp_avg_sq, numel, block_tensor, block_first, ntensors, nblocks, scratch, steps,
    # max_norm, lr, beta1, beta2, eps, weight_decay, hyper_dev, ctl, stream
    good = [P, P, P, P, P, P, P, P, 1, 1, P, P, f(0.1), f(1e-4), f(0.9), f(0.999), f(1e-8), f(1e-2), N, P, N]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 19):
        a = list(good); a[i] = N
        assert lib.effdet_clip_adamw_step_gated(*a) == EINVAL, i
    for i in (8, 9):
        for bad in (0, -1):
            a = list(good); a[i] = bad
            assert lib.effdet_clip_adamw_step_gated(*a) == EINVAL, (i, bad)


def test_accumulate_with_written_back_clipped_gradients_is_refused():
    import torch
    from efficientdet.pytorch_amd.optim import ClipAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match='write_clipped_grads'):
        ClipAdamW([p], accumulate=True, write_clipped_grads=True)
    assert ClipAdamW([p], accumulate=True).accumulate is True
    plain = ClipAdamW([p])
    assert plain.accumulate is False
    for call in (plain.loss_meter, plain.reset_epoch, lambda: plain.accumulate_grads(torch.zeros(()))):
        with pytest.raises(RuntimeError, match='accumulate=True'):
            call()
    m = ClipAdamW([p], accumulate=True).loss_meter()             # nothing built yet: np.mean([]) is NaN
    assert m[0] != m[0] and m[1:] == (0, 0, 0)


def test_graphed_train_loop_exists_and_refuses_wrapped_models_and_plain_optimizers():
    import torch
    from efficientdet.pytorch_amd import graph
    from efficientdet.pytorch_amd.optim import ClipAdamW
    assert callable(graph.GraphedTrainLoop)
    for name in ('__call__', 'epoch_mean', 'reset_epoch'):
        assert hasattr(graph.GraphedTrainLoop, name)
    lin = torch.nn.Linear(2, 2)
    x = torch.zeros(1)
    with pytest.raises(NotImplementedError, match='DataParallel'):
        graph.GraphedTrainLoop(torch.nn.DataParallel(lin), ClipAdamW(lin.parameters(), accumulate=True), x, x)
    with pytest.raises(RuntimeError, match='accumulate=True'):
        graph.GraphedTrainLoop(lin, ClipAdamW(lin.parameters()), x, x)


def test_documents_name_the_class_where_they_speak_of_accumulation():
    md = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'works through the custom autograd nodes' not in md
    lines = [l for l in md.splitlines() if 'grad_accumulation_steps' in l]
    assert lines
    for l in lines:
        assert 'GraphedTrainLoop' in l, l[:160]
    assert 'train.py:104-133' in md
    assert 'GraphedTrainLoop' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'GraphedTrainLoop' in open(os.path.join(ROOT, 'README.md')).read()
