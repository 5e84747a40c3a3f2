"""CPU tier: the return codes with which the detection-loss entry points refuse a call before anything is enqueued, and which refusal
wins where several apply.  All 24 loss exports of csrc/loss.hip are covered: the 19 that launch (effdet_focal_loss_*, effdet_box_loss_*,
effdet_loss_opts_*, effdet_loss_atss_*, effdet_loss_quality_*, effdet_loss_tal_fwd / _fwd_grad) and the five *_workspace_bytes
(effdet_loss_tal_metrics and effdet_positive_pixel_map are not part of the family).  The tensor pointers are one host buffer's address
and are never dereferenced: every row is refused before the first HIP call.  The expected codes are those of the library before the
loss launches went through one call record (recorded there; this file passed against it unchanged).

Rows that are NOT listed because the call would launch (the entry point does not make that check, and the refactor does not add it):
  B / A / num_classes = 0 alone on effdet_focal_loss_fwd / _fwd_grad and effdet_box_loss_fwd / _fwd_grad (listed with N = 0 added);
  B = 0 alone on effdet_loss_opts_bwd_reg with a box kind (listed with a null dreg added), and N = 0 there;
  B = 0, B = 65536, A = 0, N = 0 on effdet_focal_loss_bwd / _bwd_pix / _bwd_reg and effdet_box_loss_bwd_reg (none of them is checked);
  a null quality struct on effdet_loss_tal_fwd / _fwd_grad, and a null atss on effdet_loss_quality_fwd / _fwd_grad (both are valid calls)."""
import ctypes as C

EINVAL, EUNSUPPORTED = -1, -3
B0, A0, NC0, N0 = 3, 261, 4, 2                    # A = 252 + 9: two pyramid levels
BIG = 1 << 40
ROWS = 658                                        # rows of the table below

LAYOUT = {'fwd': 'cls reg anchors annots losses ws ws_bytes B A nc N',
          'fwd_grad': 'cls reg anchors annots losses ws ws_bytes dcls dld dtype B A nc N',
          'bwd': 'cls reg anchors annots gscale ws dcls dreg dtype B A nc N',
          'bwd_pix': 'cls reg anchors annots gscale ws dcls dld dreg dtype B A nc N',
          'bwd_reg': 'reg anchors annots gscale ws dreg reg_ld dtype B A N',
          'bwd_cls': 'cls annots gscale ws dcls dld dtype B A nc N'}
POINTERS = ('cls', 'reg', 'anchors', 'annots', 'losses', 'gscale', 'ws', 'dcls', 'dreg')
EXTRA = {'focal_loss': '', 'box_loss': 'kind weight', 'loss_opts': 'opts', 'loss_atss': 'opts atss', 'loss_quality': 'opts atss ql',
         'loss_tal': 'opts tal ql'}
STEMS = {'focal_loss': ('fwd', 'fwd_grad', 'bwd', 'bwd_pix', 'bwd_reg'), 'box_loss': ('fwd', 'fwd_grad', 'bwd_reg'),
         'loss_opts': ('fwd', 'fwd_grad', 'bwd_cls', 'bwd_reg'), 'loss_atss': ('fwd', 'fwd_grad'),
         'loss_quality': ('fwd', 'fwd_grad', 'bwd_cls'), 'loss_tal': ('fwd', 'fwd_grad')}
ENTRIES = [(fam, stem) for fam in STEMS for stem in STEMS[fam]]
WORKSPACE = ['effdet_loss_workspace_bytes', 'effdet_loss_opts_workspace_bytes', 'effdet_loss_atss_workspace_bytes',
             'effdet_loss_quality_workspace_bytes', 'effdet_loss_tal_workspace_bytes']


def al256(n):
    return (n + 255) // 256 * 256


def layout_bytes(B, A, nc, N):
    """The five workspace layouts written out (include/effdet_hip.h, effdet_loss_opts.h, effdet_atss.h, effdet_quality_loss.h,
    effdet_tal.h): every buffer rounded up to 256 bytes."""
    na = (A + 255) // 256
    ncb = ((A * nc + 3) // 4 + (A // 9 + 1) * 16 + 1023) // 1024 + 1
    plain = al256(4 * B * A) + al256(4 * B * 32) + al256(4 * B * na) + al256(4 * B * ncb)       # assign, stat, part_reg, part_cls
    opts = plain + al256(4 * B * N) + 2 * al256(4 * B * A)                                     # gtmax, best, barg
    atss = plain + al256(8 * B * N * 8) + al256(4 * B * N)                                     # kth, thr
    quality = max(opts, atss) + al256(4 * B * A)                                               # q
    tal = quality + al256(8 * B * N * 16) + al256(4 * B * N * 2) + al256(8 * B * A)            # keys, (mmax, umax), claims
    return {'focal_loss': plain, 'box_loss': plain, 'loss_opts': opts, 'loss_atss': atss, 'loss_quality': quality, 'loss_tal': tal}


def test_refusal_table_of_the_loss_entry_points():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    names = ['effdet_%s_%s' % e for e in ENTRIES]
    assert len(names) == 19
    L = _lib.require(*(names + WORKSPACE))
    buf = C.create_string_buffer(512)
    P = (C.addressof(buf) + 127) & ~127           # the one address every tensor gets (128-byte aligned: the split layout's rule)
    nan = float('nan')

    def opts(**kw):
        v = dict(alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=1.0 / 9.0, reg_weight=1.0, pos_iou=0.5, neg_iou=0.4, low_quality=0,
                 box_kind=0, box_weight=1.0)
        v.update(kw)
        return _lib.LossOpts(**v)

    def atss(A=A0, topk=9, num_levels=2, start=None):
        t = _lib.Atss(topk, num_levels)
        for i, v in enumerate(start if start is not None else (0, A - 9, A)):
            t.level_start[i] = v
        return t

    tal = lambda **kw: _lib.Tal(**dict(dict(topk=13, alpha=1.0, beta=6.0, aligned_target=0), **kw))
    ql = lambda **kw: _lib.QualityLoss(**dict(dict(kind=_lib.QUALITY_QFL, beta=2.0, alpha=0.75, gamma=2.0), **kw))
    ref = lambda s: None if s is None else C.byref(s)

    def need(fam, B=B0, A=A0, nc=NC0, N=N0, with_atss=True):
        if fam in ('focal_loss', 'box_loss'):
            return int(L.effdet_loss_workspace_bytes(B, A, nc))
        if fam == 'loss_opts':
            return int(L.effdet_loss_opts_workspace_bytes(B, A, nc, N))
        if fam == 'loss_atss':
            return int(L.effdet_loss_atss_workspace_bytes(B, A, nc, N, ref(atss(A))))
        if fam == 'loss_quality':
            return int(L.effdet_loss_quality_workspace_bytes(B, A, nc, N, ref(atss(A)) if with_atss else None))
        return int(L.effdet_loss_tal_workspace_bytes(B, A, nc, N, ref(tal())))

    def call(fam, stem, **kw):
        """The entry point effdet_<fam>_<stem> on the valid base call with kw replaced."""
        a = dict(B=B0, A=A0, nc=NC0, N=N0, ws_bytes=BIG, dtype=_lib.F32, dld=0 if stem == 'bwd_cls' else 64, reg_ld=0, kind=2, weight=1.0,
                 ql=ql() if fam == 'loss_quality' else None)
        a.update({p: P for p in POINTERS})
        a.update(kw)
        for k, make in (('opts', opts), ('tal', tal)):
            if k not in a:
                a[k] = make()
        if 'atss' not in a:
            a['atss'] = atss(a['A'])
        extra = EXTRA[fam].split()
        if (fam, stem) == ('loss_quality', 'bwd_cls'):
            extra = ['opts', 'ql']
        elif stem in ('bwd_reg', 'bwd_cls'):
            extra = [e for e in extra if e in ('kind', 'weight', 'opts')]
        args = [a[n] for n in LAYOUT[stem].split()] + [ref(a[e]) if e in ('opts', 'atss', 'tal', 'ql') else a[e] for e in extra]
        return int(getattr(L, 'effdet_%s_%s' % (fam, stem))(*args, None))

    got = {}

    def row(what, rc, want):
        assert what not in got, what
        got[what] = (int(rc), want)

    FWD = [e for e in ENTRIES if e[1] in ('fwd', 'fwd_grad')]                       # the ten forward calls
    FWD_GRAD = [e for e in FWD if e[1] == 'fwd_grad']
    OPTS_FWD = [e for e in FWD if e[0] not in ('focal_loss', 'box_loss')]           # ... that take the options struct
    BWD_CLS = [('loss_opts', 'bwd_cls'), ('loss_quality', 'bwd_cls')]
    BWD_REG = [e for e in ENTRIES if e[1] == 'bwd_reg']
    WITH_OPTS = OPTS_FWD + BWD_CLS + [('loss_opts', 'bwd_reg')]
    WITH_ATSS = [e for e in FWD if e[0] in ('loss_atss', 'loss_quality')]
    WITH_TAL = [e for e in FWD if e[0] == 'loss_tal']
    WITH_QL = [e for e in ENTRIES if e[0] == 'loss_quality'] + WITH_TAL
    DCLS = FWD_GRAD + [('focal_loss', 'bwd_pix')] + BWD_CLS                         # a pixel-major d(cls) output
    NO_SPLIT = [('focal_loss', 'bwd'), ('focal_loss', 'bwd_pix')] + BWD_CLS         # d(cls) outputs without the split layout
    name = lambda e: '%s_%s' % e
    box_opts = lambda **kw: opts(box_kind=2, box_weight=2.0, **kw)

    # ---- null tensors, one at a time: EINVAL
    for e in ENTRIES:
        for t in LAYOUT[e[1]].split():
            if t in POINTERS:
                row('%s null %s' % (name(e), t), call(*e, **{t: None}), EINVAL)
    for t in ('reg', 'anchors', 'annots', 'gscale', 'ws', 'dreg'):
        row('loss_opts_bwd_reg, box kind, null %s' % t, call('loss_opts', 'bwd_reg', opts=box_opts(), **{t: None}), EINVAL)

    # ---- workspace one byte short of the export's own answer, for each of the five layouts
    for e in FWD:
        row('%s workspace one byte short' % name(e), call(*e, ws_bytes=need(e[0]) - 1), EINVAL)
        if e[0] == 'loss_quality':
            row('%s without atss, workspace one byte short' % name(e), call(*e, atss=None, ws_bytes=need(e[0], with_atss=False) - 1), EINVAL)
        if e[0] == 'loss_tal':
            row('%s with a quality loss, workspace one byte short' % name(e), call(*e, ql=ql(), ws_bytes=need(e[0]) - 1), EINVAL)
    row('loss_quality_fwd, workspace of the bands alone', call('loss_quality', 'fwd', atss=None, ws_bytes=need('loss_opts')), EINVAL)
    row('loss_quality_fwd, workspace of ATSS alone', call('loss_quality', 'fwd', ws_bytes=need('loss_atss')), EINVAL)
    row('loss_tal_fwd, workspace of a quality loss', call('loss_tal', 'fwd', ws_bytes=need('loss_quality')), EINVAL)
    row('loss_opts_fwd, workspace of the defaults', call('loss_opts', 'fwd', ws_bytes=need('focal_loss')), EINVAL)
    row('focal_loss_fwd, no workspace bytes', call('focal_loss', 'fwd', ws_bytes=0), EINVAL)

    # ---- B = 65536, N = 0 on every entry point that checks them
    for e in FWD + BWD_CLS:
        row('%s B 65536' % name(e), call(*e, B=65536), EINVAL)
        row('%s N 0' % name(e), call(*e, N=0), EINVAL)
    row('loss_opts_bwd_reg N 0', call('loss_opts', 'bwd_reg', N=0), EINVAL)

    # ---- B / A / num_classes = 0: where they are checked, and (with another refusal) where they are not
    for e in OPTS_FWD + BWD_CLS:
        for k in ('B', 'A', 'nc'):
            row('%s %s 0' % (name(e), k), call(*e, **{k: 0}), EINVAL)
    for k in ('B', 'A'):
        row('loss_opts_bwd_reg %s 0' % k, call('loss_opts', 'bwd_reg', **{k: 0}), EINVAL)
        row('loss_opts_bwd_reg, box kind, %s 0 and null dreg' % k, call('loss_opts', 'bwd_reg', opts=box_opts(), dreg=None, **{k: 0}), EINVAL)
    for e in FWD:
        if e[0] in ('focal_loss', 'box_loss'):
            for k in ('B', 'A', 'nc'):
                row('%s %s 0 and N 0' % (name(e), k), call(*e, N=0, **{k: 0}), EINVAL)
    for e in BWD_CLS:
        row('%s negative dld' % name(e), call(*e, dld=-4), EINVAL)

    # ---- the four structs: null where the entry point needs one, and each invalid field
    for e in WITH_OPTS:
        row('%s null opts' % name(e), call(*e, opts=None), EINVAL)
        for k, v in (('alpha', 0.0), ('gamma', 9.0), ('label_smoothing', 1.0), ('beta', 0.0), ('reg_weight', -1.0), ('pos_iou', 1.5),
                     ('neg_iou', 0.6), ('low_quality', 2), ('box_kind', 5), ('box_weight', nan)):
            row('%s opts %s %r' % (name(e), k, v), call(*e, opts=opts(**{k: v})), EINVAL)
    for e in WITH_ATSS:
        if e[0] == 'loss_atss':
            row('%s null atss' % name(e), call(*e, atss=None), EINVAL)
        for what, t in (('topk 0', atss(topk=0)), ('topk 17', atss(topk=17)), ('num_levels 0', atss(num_levels=0)),
                        ('num_levels 9', atss(num_levels=9)), ('first start 1', atss(start=(1, 252, 261))),
                        ('last start not A', atss(start=(0, 252, 260))), ('empty level', atss(start=(0, 0, 261))),
                        ('levels of another A', atss(A=270))):
            row('%s atss %s' % (name(e), what), call(*e, atss=t), EINVAL)
        row('%s low_quality 1' % name(e), call(*e, opts=opts(low_quality=1)), EINVAL)
    for e in WITH_TAL:
        row('%s null tal' % name(e), call(*e, tal=None), EINVAL)
        for k, v in (('topk', 0), ('topk', 17), ('alpha', 5.0), ('alpha', nan), ('beta', 17.0), ('aligned_target', 2)):
            row('%s tal %s %r' % (name(e), k, v), call(*e, tal=tal(**{k: v})), EINVAL)
        row('%s low_quality 1' % name(e), call(*e, opts=opts(low_quality=1)), EINVAL)
    for e in WITH_QL:
        if e[0] == 'loss_quality':
            row('%s null quality' % name(e), call(*e, ql=None), EINVAL)
        for k, v in (('kind', 0), ('kind', 3), ('beta', 0.5), ('alpha', 0.0), ('gamma', 9.0), ('gamma', nan)):
            row('%s quality %s %r' % (name(e), k, v), call(*e, ql=ql(**{k: v})), EINVAL)

    # ---- the stand-alone box term
    for stem in STEMS['box_loss']:
        for k, v in (('kind', 0), ('kind', 5), ('weight', -1.0), ('weight', nan)):
            row('box_loss_%s %s %r' % (stem, k, v), call('box_loss', stem, **{k: v}), EINVAL)

    # ---- the d(cls) output
    for e in FWD_GRAD + NO_SPLIT:
        for v in (_lib.F32_BF16X3, 7):
            row('%s dtype %d' % (name(e), v), call(*e, dtype=v), EINVAL)
    for e in NO_SPLIT:
        row('%s split' % name(e), call(*e, dtype=_lib.F32_SPLIT, dld=0 if e[1] == 'bwd' else 64), EINVAL)
    for e in FWD_GRAD + [('focal_loss', 'bwd_pix')]:
        for v in (0, -4):
            row('%s dld %d' % (name(e), v), call(*e, dld=v), EINVAL)
    for e in DCLS:
        row('%s dld %% 4' % name(e), call(*e, dld=38), EINVAL)
        row('%s nc %% 4' % name(e), call(*e, nc=3, dld=64), EINVAL)
        row('%s A %% 9' % name(e), call(*e, A=262, dld=64), EINVAL)
        row('%s dld < 9 nc' % name(e), call(*e, dld=32), EINVAL)
    for e in FWD_GRAD:
        row('%s split, dld %% 32' % name(e), call(*e, dtype=_lib.F32_SPLIT, dld=36), EINVAL)
        row('%s split, dcls not 128-byte aligned' % name(e), call(*e, dtype=_lib.F32_SPLIT, dcls=P + 4), EINVAL)

    # ---- the d(reg) output
    for e, kw in [(e, {}) for e in BWD_REG] + [(('loss_opts', 'bwd_reg'), dict(opts=box_opts()))]:
        what = name(e) + (', box kind,' if kw else '')
        for v in (_lib.F32_BF16X3, 7):
            row('%s dtype %d' % (what, v), call(*e, dtype=v, **kw), EINVAL)
        row('%s reg_ld 32' % what, call(*e, reg_ld=32, **kw), EINVAL)
        row('%s reg_ld %% 4' % what, call(*e, reg_ld=38, **kw), EINVAL)
        row('%s A %% 9 with reg_ld' % what, call(*e, A=262, reg_ld=64, **kw), EINVAL)
        row('%s split, reg_ld 0' % what, call(*e, dtype=_lib.F32_SPLIT, **kw), EINVAL)
        row('%s split, reg_ld %% 32' % what, call(*e, dtype=_lib.F32_SPLIT, reg_ld=36, **kw), EINVAL)
        row('%s split, dreg not 128-byte aligned' % what, call(*e, dtype=_lib.F32_SPLIT, reg_ld=64, dreg=P + 4, **kw), EINVAL)

    # ---- EUNSUPPORTED: an extent past 2^31 with everything else valid (the workspace byte count is the export's own answer for that
    # shape), and the same with one EINVAL condition added, which wins
    ABIG = 9 * 59652324                           # A * 4 classes >= 2^31 (and (A / 9) * 64 as well)
    APIX = 9 << 22                                # A * 4 classes < 2^31, (A / 9) * 512 = 2^31
    for e in FWD:
        kw = dict(A=ABIG, ws_bytes=need(e[0], A=ABIG))
        row('%s A nc >= 2^31' % name(e), call(*e, **kw), EUNSUPPORTED)
        row('%s A nc >= 2^31, N 0' % name(e), call(*e, N=0, **kw), EINVAL)
        row('%s A nc >= 2^31, null cls' % name(e), call(*e, cls=None, **kw), EINVAL)
        row('%s A nc >= 2^31, workspace one byte short' % name(e), call(*e, A=ABIG, ws_bytes=kw['ws_bytes'] - 1), EINVAL)
    for e in FWD_GRAD:
        kw = dict(A=APIX, dld=512, ws_bytes=need(e[0], A=APIX))
        row('%s (A / 9) dld >= 2^31' % name(e), call(*e, **kw), EUNSUPPORTED)
        row('%s (A / 9) dld >= 2^31, null losses' % name(e), call(*e, losses=None, **kw), EINVAL)
        row('%s (A / 9) dld >= 2^31, split, dcls not 128-byte aligned' % name(e), call(*e, dtype=_lib.F32_SPLIT, dcls=P + 4, **kw), EINVAL)
        row('%s A nc >= 2^31, dtype 7' % name(e), call(*e, A=ABIG, ws_bytes=need(e[0], A=ABIG), dtype=7), EINVAL)
    for e in BWD_CLS:
        row('%s A nc >= 2^31' % name(e), call(*e, A=ABIG), EUNSUPPORTED)
        row('%s A nc >= 2^31, null gscale' % name(e), call(*e, A=ABIG, gscale=None), EINVAL)
        row('%s A nc >= 2^31, B 65536' % name(e), call(*e, A=ABIG, B=65536), EINVAL)
        row('%s A nc >= 2^31, gamma 9' % name(e), call(*e, A=ABIG, opts=opts(gamma=9.0)), EINVAL)
    row('loss_quality_bwd_cls A nc >= 2^31, quality kind 0', call('loss_quality', 'bwd_cls', A=ABIG, ql=ql(kind=0)), EINVAL)
    for e in BWD_CLS + [('focal_loss', 'bwd_pix')]:
        row('%s (A / 9) dld >= 2^31' % name(e), call(*e, A=APIX, dld=512), EUNSUPPORTED)
        row('%s (A / 9) dld >= 2^31, null dcls' % name(e), call(*e, A=APIX, dld=512, dcls=None), EINVAL)
        row('%s (A / 9) dld >= 2^31, split' % name(e), call(*e, A=APIX, dld=512, dtype=_lib.F32_SPLIT), EINVAL)
    for fam in ('loss_atss', 'loss_quality', 'loss_tal'):
        row('%s_fwd A nc >= 2^31, low_quality 1' % fam, call(fam, 'fwd', A=ABIG, ws_bytes=need(fam, A=ABIG), opts=opts(low_quality=1)), EINVAL)
    row('box_loss_fwd A nc >= 2^31, kind 0', call('box_loss', 'fwd', A=ABIG, ws_bytes=need('box_loss', A=ABIG), kind=0), EINVAL)

    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not wrong and len(got) == ROWS, (wrong, len(got))

    # ---- the five workspace-size exports: the layout arithmetic, and -1 for the invalid structs
    for shape in ((B0, A0, NC0, N0), (2, 49104, 20, 7)):
        want = layout_bytes(*shape)
        B, A, nc, N = shape
        for fam in want:
            assert need(fam, B, A, nc, N) == want[fam], (fam, shape)
        assert need('loss_quality', B, A, nc, N, with_atss=False) == want['loss_quality']
    assert layout_bytes(B0, A0, NC0, N0) == {'focal_loss': 4352, 'box_loss': 4352, 'loss_opts': 11264, 'loss_atss': 5120,
                                             'loss_quality': 14592, 'loss_tal': 22016}
    sized = lambda fn, s: int(getattr(L, fn)(B0, A0, NC0, N0, ref(s)))
    assert sized('effdet_loss_atss_workspace_bytes', None) == -1 and sized('effdet_loss_tal_workspace_bytes', None) == -1
    assert sized('effdet_loss_quality_workspace_bytes', None) == 14592                # a null atss: the bands
    for t in (atss(topk=0), atss(topk=17), atss(num_levels=0), atss(num_levels=9), atss(start=(1, 252, 261)), atss(start=(0, 252, 260)),
              atss(start=(0, 0, 261))):
        assert sized('effdet_loss_atss_workspace_bytes', t) == -1 and sized('effdet_loss_quality_workspace_bytes', t) == -1
    for t in (tal(topk=0), tal(topk=17), tal(alpha=5.0), tal(beta=nan), tal(aligned_target=2)):
        assert sized('effdet_loss_tal_workspace_bytes', t) == -1

