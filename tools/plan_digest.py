"""digest of what the host planner decides (CPU only, no device): for the three builds x a fixed layer list, a short SHA-1 of the
raw bytes of every planned descriptor and the kernel family of each role.  Descriptors hold no pointers at plan time, so two
trees whose planners agree print byte-identical JSON.
--routes prints instead what the host dispatch decides: every planned forward, data-gradient and weight-gradient descriptor is filled
with fake non-null addresses (the entry points asked are host-only and never dereference) over the prologue modes, the optional
operands / epilogues and both storage types of either tensor, and each sisr_*_eligible / *_parts / *_bnb_parts / *_slabs / *_slab_lead answer is
printed, with engine.can_fuse_bn_backward per layer.  Run it under each A/B switch (SISR_TRUNK=0, ...): two trees that route alike
print byte-identical JSON.
--weights prints how engine._layout_weights lays the packed weight images of the layer list out, per build and with / without the
data gradient: every image's (buffer, offset, fp32 slots rounded up to the 16 bytes the next piece starts on) and the sizes of
the buffers.  Two trees that lay out alike print byte-identical JSON.
--wgrad prints which launch engine.WgradDeepBatch().add keeps every layer's weight gradient for -- alone, wgrad_deep.hip's batch or the
persistent trunk kernel's, with the key of its group in the batch -- over the x prologues none / affine-act and the gradient prologues
of the layer (operands of one-element host tensors: add() reads their address, type and modes only).  Run it under each batching
switch (SISR_WGRAD_BATCH=0, SISR_WGRAD_BATCH_TRUNK_PIXELS=0, ...): two trees that batch alike print byte-identical JSON.
usage: python tools/plan_digest.py [--routes | --weights | --wgrad] [root of the tree whose package is digested; default: this one]"""
import ctypes as C, hashlib, importlib, itertools, json, os, sys, types
MODES = ('--routes', '--weights', '--wgrad')
ROUTES, WEIGHTS, WGRAD = (m in sys.argv[1:] for m in MODES)
_args = [a for a in sys.argv[1:] if a not in MODES]
ROOT = os.path.abspath(_args[0] if _args else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
E = importlib.import_module('single-image-super-resolution_amd.engine')

from plan_layers import LAYERS                   # beside this file


def sha(desc):
    return hashlib.sha1(bytes(desc)).hexdigest()[:12]


def dgrad(d):
    """the data-gradient plan in whichever of its four shapes"""
    if d is None:
        return None
    if isinstance(d, list):                       # four parity classes: (desc, r0y, r0x, kind) | None
        return [None if c is None else [sha(c[0]), c[1], c[2], int(c[3])] for c in d]
    if hasattr(d, 'classes'):                     # one launch over the four classes: (taps y, taps x, r0y, r0x) each
        return {'desc': sha(d.desc), 'classes': [[int(v) for v in c] for c in d.classes]}
    return sha(d)


FAKE = 0x7f0000001000            # never dereferenced
CONV_ASK = ('sisr_conv2d_trunk_eligible', 'sisr_conv2d_trunk_f32_eligible', 'sisr_conv2d_thin_eligible', 'sisr_conv2d_toimage_eligible',
            'sisr_conv2d_toimage_f32_eligible', 'sisr_conv2d_deep_eligible', 'sisr_conv2d_bf16_parts', 'sisr_conv2d_f32_parts',
            'sisr_conv2d_f32_bnb_parts')
WGRAD_ASK = ('sisr_wgrad_trunk_eligible', 'sisr_wgrad_trunk_f32_eligible', 'sisr_wgrad_thin_eligible', 'sisr_wgrad_toimage_eligible',
             'sisr_wgrad_toimage_f32_eligible', 'sisr_wgrad_deep_eligible', 'sisr_wgrad_bf16_slabs', 'sisr_wgrad_f32_slabs',
             'sisr_wgrad_bf16_slab_lead')


def ask(lib, names, d):
    return ','.join(str(int(getattr(lib, n)(C.byref(d)))) for n in names)


def conv_routes(lib, L, desc, kind, modes):
    """answers for one planned conv descriptor: {prologue, x_mode, y_mode, epilogue, storage: one answer per combination of res,
    bias, stat_part, bnb_part + bnb_x and the fin_* block}"""
    res = {}
    pros = [(str(m), m, True) for m in range(8)] + [('7 bare', L.PRO_RES_AFFINE, False)]
    for (name, pro, operands), (x_mode, y_mode, epi), x_bf, y_bf in itertools.product(pros, modes, (0, 1), (0, 1)):
        rows = []
        for has_res, has_bias, has_stat, has_bnb, has_fin in itertools.product((0, 1), repeat=5):
            d = type(desc).from_buffer_copy(desc)
            d.x1 = d.y = FAKE
            d.x_mode, d.y_mode, d.epi_act, d.pro_mode, d.mfma_split = x_mode, y_mode, epi, pro, E.mfma_split()
            d.x_bf16, d.y_bf16, d.res_bf16, d.bnbx_bf16 = x_bf, y_bf, y_bf, y_bf
            if E.Kind(kind).deep:
                d.wdeep = d.deep_ws = FAKE
                for c in range(4):
                    d.wdeep_c[c] = FAKE
            else:
                d.wpk = FAKE
            if operands:
                d.x2 = d.x_out = d.pa = d.pb = d.pd = d.ps = d.pt = FAKE
            if has_res:
                d.res = FAKE
            if has_bias:
                d.bias = FAKE
            if has_stat:
                d.stat_part = d.cnt_part = FAKE
            if has_bnb:
                d.bnb_part = d.bnb_x = d.bnb_scale = d.bnb_shift = d.bnb_mean = d.bnb_invstd = FAKE
            if has_fin:
                d.fin_stat = d.fin_cnt = d.fin_gamma = d.fin_beta = d.fin_rm = d.fin_rv = d.fin_k = FAKE
                d.fin_rows = 4
            rows.append(ask(lib, CONV_ASK, d))
        res['pro %s x%d y%d epi%d bf%d%d' % (name, x_mode, y_mode, epi, x_bf, y_bf)] = ' '.join(rows)
    return res


def wgrad_routes(lib, L, desc):
    """answers for the planned weight-gradient descriptor over both prologues, the operand layouts and the storage flags"""
    res = {}
    gpros = (L.PRO_NONE, L.PRO_BNBWD, L.PRO_BNACT_BWD, L.PRO_ACT_BWD, L.PRO_TANH_BWD)
    for x_mode, g_mode in itertools.product((L.X_NHWC, L.X_NCHW), (L.X_NHWC, L.X_NCHW, L.X_UNSHUFFLE2)):
        rows = []
        for x_bf, g_bf, pro, gpro in itertools.product((0, 1), (0, 1), (L.PRO_NONE, L.PRO_ACT, L.PRO_AFFINE_ACT), gpros):
            d = type(desc).from_buffer_copy(desc)
            d.x1 = d.g1 = d.g2 = d.slab = d.bias_slab = d.pa = d.pd = d.qa = d.qb = d.qd = d.qs = d.qt = FAKE
            d.x_mode, d.g_mode, d.x_bf16, d.g_bf16, d.pro_mode, d.gpro_mode = x_mode, g_mode, x_bf, g_bf, pro, gpro
            d.mfma_split = E.mfma_split()
            rows.append(ask(lib, WGRAD_ASK, d))
        res['x%d g%d' % (x_mode, g_mode)] = ' '.join(rows)
    return res


def routes(geom, f, d, g, kinds):
    L = E.L
    lib = L.lib()
    image_in, image_out = (L.X_NCHW, L.Y_NHWC, L.EPI_NONE), [(L.X_NHWC, L.Y_NCHW, e) for e in (L.EPI_NONE, L.EPI_TANH)]
    out = {'f': conv_routes(lib, L, f, kinds[0], [(L.X_NHWC, f.y_mode, L.EPI_NONE)] + [image_in] * (geom.cin == 3) + image_out * (geom.cout == 3))}
    shape = E._dgrad_shape(d)
    if shape == E.DG_CONV:
        # (the upscale conv's data gradient reads the un-shuffling view of the gradient)
        out['d'] = conv_routes(lib, L, d, kinds[1], [(L.X_UNSHUFFLE2 if geom.shuffle2 else L.X_NHWC, L.Y_NHWC, L.EPI_NONE)])
    elif shape == E.DG_X4:
        out['d'] = conv_routes(lib, L, d.desc, kinds[1], [(L.X_NHWC, L.Y_NHWC, L.EPI_NONE)])
    elif shape == E.DG_CLASSES:
        out['d'] = [None if c is None else conv_routes(lib, L, c.desc, c.kind, [(L.X_NHWC, L.Y_NHWC, L.EPI_NONE)]) for c in d]
    out['g'] = wgrad_routes(lib, L, g)
    prep = types.SimpleNamespace(plans=(f, d, g), kinds=kinds, ref=types.SimpleNamespace(geom=geom))
    out['can_fuse_bn_backward'] = bool(E.can_fuse_bn_backward(prep))
    return out


def weights(need_dgrad):
    """the layer list as ONE table (offsets run on from layer to layer)"""
    items = [(E.ConvRef(E.ConvGeom(cin, cout, k, stride, shuffle2=sh, deep_dgrad=dd), None, None), n, h, w)
             for cin, cout, k, stride, sh, dd, n, h, w in LAYERS]
    _, offs, sizes = E._layout_weights(items, need_dgrad)
    layers = [{'images': [[i.buf, i.off, (i.slots + 3) & ~3] for i in imgs if i is not None], 's': [s0, s1]} for imgs, s0, s1 in offs]
    return {'layers': layers, 'sizes': sizes}


def wgrad_batches(geom, g, kinds, n, h, w):
    """{x prologue, gradient prologue: 'alone' | 'deep <group key>' | 'trunk <group key>'}"""
    import torch
    L = E.L
    prep = types.SimpleNamespace(plans=(None, None, g), kinds=kinds, ref=types.SimpleNamespace(geom=geom))
    ho, wo = geom.out_hw(h, w)
    one = lambda dt: torch.zeros(1, dtype=dt)
    c = one(torch.float32)
    x = one(torch.float32 if geom.cin == 3 else E.act_dtype(geom.cin))
    x_mode = L.X_NCHW if geom.cin == 3 else L.X_NHWC                     # (the 3-channel image is NCHW fp32)
    if geom.shuffle2:                                                     # the upscale conv: the gradient behind the PixelShuffle
        g_mode, g_t, gpros = L.X_UNSHUFFLE2, one(E.act_dtype(geom.cout // 4)), (L.PRO_ACT_BWD,)
    elif geom.cout == 3:                                                  # the last conv: the NCHW fp32 image gradient
        g_mode, g_t, gpros = L.X_NCHW, c, (L.PRO_TANH_BWD,)
    else:
        g_mode, g_t, gpros = L.X_NHWC, one(E.act_dtype(geom.cout)), (L.PRO_NONE, L.PRO_BNBWD, L.PRO_BNACT_BWD, L.PRO_ACT_BWD)
    res = {}
    for pro, gpro in itertools.product((L.PRO_NONE, L.PRO_AFFINE_ACT), gpros):
        x_op = E.Operand(x, (n, h, w, geom.cin), pro=pro, mode=x_mode, pa=c, pd=c, slope=1.0)
        g_op = E.Operand(g_t, (n, ho, wo, geom.cout), pro=gpro, mode=g_mode, x2=g_t, pa=c, pb=c, pd=c, ps=c, pt=c, slope=0.2)
        wb = E.WgradDeepBatch()
        red = wb.add(prep, x_op, g_op)
        assert (red is None) == (not wb.items and not wb.trunk) and len(wb.items) + len(wb.trunk) <= 1
        # (a member is (prepared layer, filled descriptor, ...): the keys are the engine's own)
        where = 'alone'
        for m in wb.items:
            where = 'deep %s' % (tuple(int(v) for v in E._deep_batch_key(m[1])),)
        for m in wb.trunk:
            where = 'trunk %s' % (tuple(int(v) for v in E._trunk_batch_key(m[0], m[1])),)
        res['pro %d gpro %d' % (pro, gpro)] = where
    return res


out = {}
for build in ('fp32', 'bf16x3', 'bf16'):
    E.set_precision(build)
    if WEIGHTS:
        out[build] = {'with dgrad': weights(True), 'forward only': weights(False)}
        continue
    for cin, cout, k, stride, shuffle2, deep_dgrad, n, h, w in LAYERS:
        geom = E.ConvGeom(cin, cout, k, stride, shuffle2=shuffle2, deep_dgrad=deep_dgrad)
        f, d, g, kinds = geom.plans(n, h, w)
        out['%s %d>%d k%d s%d%s%s %dx%dx%d' % (build, cin, cout, k, stride, ' up' * shuffle2, ' vgg' * deep_dgrad, n, h, w)] = \
            routes(geom, f, d, g, kinds) if ROUTES else wgrad_batches(geom, g, kinds, n, h, w) if WGRAD else {'f': sha(f), 'd': dgrad(d), 'g': sha(g), 'kinds': [int(v) for v in kinds]}
print(json.dumps(out, indent=1, sort_keys=True))
