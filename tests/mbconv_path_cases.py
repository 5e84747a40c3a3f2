"""The runs of the MBConv call-sequence pin, shared by its GPU test (tests/test_gpu_mbconv_call_sequence.py, which records and compares)
and by the host test of the path functions (tests/test_mbconv_path_host.py, which predicts), and the fixture's file format.

Shape: D0, 8 classes, B = 4 @512, drop_connect 0.2 with injected masks (the row scale is live) -- the smallest batch at which every
fused kernel appears: pw_dgrad_se needs M >= 65 536 at Co 24 (4 x 128^2), pw_bwd M >= 131 072 at Cin 16 (block 1 reads 4 x 256^2); the
maps run from 256^2 down to 4^2, across functional.GATE_OPERAND_MIN_HW, the `% 128` rule and the `Ho * Wo > 64` rule."""
import json
import os

HEADLINE = 'f32_hf16x3_bwd_bf16x3'
NET, NC, B, S = 'efficientdet-d0', 8, 4, 512
NBLOCKS = 16
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mbconv_call_sequence.json')

# the functions of ops that functional.mbconv_fwd / mbconv_bwd reach
OPS = ('conv2d', 'conv2d_wgrad', 'channel_scale', 'dwconv_fwd', 'expand_dw_fwd', 'dwconv_bwd', 'dwconv_wgrad', 'dwconv_dgrad',
       'dw_unpack_wgrad_bn', 'unpack_wgrad_bn', 'se_gate_fwd', 'se_gate_bwd', 'se_dgate', 'se_dgate_from_wgrad', 'se_bwd_apply', 'act_bwd',
       'pw_bwd', 'pw_dgrad_se', 'pack_weight', 'scale_pack_weight', 'dw_pack_weight', 'bn_fold')

# the switches of functional.py that the MBConv section reads ('STEM_LINK' is efficientdet.STEM_LINK)
SWITCHES = ('DW_SAVE_Y', 'EXPAND_Z_ONLY', 'SE_FUSED', 'DW_BWD_FUSED', 'PW_BWD_FUSED', 'PW_DGRAD_SE', 'FUSE_EXPAND_DW', 'FUSE_CIN',
            'GATE_IN_WEIGHTS', 'GATE_IN_WEIGHTS_TRAIN', 'GATE_IN_OPERAND', 'GATE_OPERAND_MIN_HW')


def _run(arith=HEADLINE, storage='f32', train=True, before=None, between=None):
    """before: {switch: value} set for the whole step; between: set after the forward, before the backward"""
    return dict(arith=arith, storage=storage, train=train, before=before or {}, between=between or {})


RUNS = {
    'f32': _run(arith='f32'),
    HEADLINE: _run(),
    'bf16': _run(arith='f32', storage='bf16'),
    'inference': _run(arith='f32', train=False),
    'inference_bf16': _run(arith='f32', storage='bf16', train=False),
    'se_fused_off': _run(before={'SE_FUSED': False}),
    'gate_in_operand_off': _run(before={'GATE_IN_OPERAND': False}),
    'gate_in_weights_train_on': _run(before={'GATE_IN_WEIGHTS_TRAIN': True}),
    'inference_gate_in_weights_off': _run(train=False, before={'GATE_IN_WEIGHTS': False}),
    'dw_save_y_on': _run(before={'DW_SAVE_Y': True}),
    'expand_z_only_off': _run(before={'EXPAND_Z_ONLY': False}),
    'dw_bwd_fused_off': _run(before={'DW_BWD_FUSED': False}),
    'pw_bwd_fused_off': _run(before={'PW_BWD_FUSED': False}),
    'pw_dgrad_se_off': _run(before={'PW_DGRAD_SE': False}),
    'inference_fuse_expand_dw_off': _run(train=False, before={'FUSE_EXPAND_DW': False}),
    'stem_link_off': _run(before={'STEM_LINK': False}),
    'flip_gate_in_operand_off': _run(between={'GATE_IN_OPERAND': False}),
    'flip_gate_in_weights_train_then_se_fused_off': _run(before={'GATE_IN_WEIGHTS_TRAIN': True}, between={'SE_FUSED': False}),
}


def block_geometry():
    """[(block, input side)] of D0's 16 MBConv blocks @512 (the stem halves the image)"""
    from efficientdet.pytorch_amd.config import backbone_plan
    side, out = S // 2, []
    for blk in backbone_plan('efficientnet-b0')[2]:
        out.append((blk, side))
        side = (side + blk.stride - 1) // blk.stride
    return out


# The file holds every distinct entry once ('entries') and, per run, per block, the indices of its forward and backward entries: the
# 18 runs share most of their ~6000 calls, and spelled out they would be several times the size a committed file may have.
def pack_fixture(runs):
    """{run: [{'fwd': [entry, ...], 'bwd': [...]} per block]} -> the file's form"""
    table, index = [], {}

    def ref(e):
        k = json.dumps(e, sort_keys=True)
        if k not in index:
            index[k] = len(table); table.append(e)
        return index[k]
    return {'entries': table,
            'runs': {run: [{part: [ref(e) for e in blk[part]] for part in ('fwd', 'bwd')} for blk in blocks] for run, blocks in runs.items()}}


def load_fixture(path=FIXTURE):
    """-> {run: [{'fwd': [[name, rendered arguments, returned None?], ...], 'bwd': [...]} for each of the 16 blocks]}"""
    with open(path) as f:
        d = json.load(f)
    t = d['entries']
    return {run: [{part: [t[i] for i in blk[part]] for part in ('fwd', 'bwd')} for blk in blocks] for run, blocks in d['runs'].items()}
