#!/usr/bin/env python3
"""Upscale one image file with a trained generator: ``upscale_image.py checkpoint in.png out.png [--tile --halo --feather
--ensemble --ema --niqe MODEL.npz]``.

The checkpoint is the reference's (utils._save: a dict whose ``net_g`` entry is the generator's state_dict; ``--ema`` takes the
averaged weights stored beside it as ``net_g_ema``, ema.WeightEMA.shadow_state_dict).  The architecture is read off the
state_dict's keys and shapes (``arch_from_state``) and the weights are loaded tolerantly (strict=False with the reference's
coverage report).  The image is decoded and encoded with Pillow on the host; everything between runs on the MI355X
(upscale.Upscaler).  ``--niqe MODEL.npz`` (a metrics.NiqeModel file: tools/fit_niqe.py, or a BasicSR-style parameter file) also prints
the no-reference NIQE score of the output image; no HR image is needed.  Argument handling and ``arch_from_state`` need no GPU.
"""
import argparse
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'single-image-super-resolution_amd'


def _pkg(sub):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + '.' + sub)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Upscale an image with a trained SRGAN generator on the MI355X.')
    ap.add_argument('checkpoint', help="the reference's checkpoint file (torch.save of a dict with a 'net_g' state_dict)")
    ap.add_argument('input', help='image file to upscale (anything Pillow reads; converted to RGB)')
    ap.add_argument('output', help='image file to write (format from the suffix)')
    ap.add_argument('--tile', type=int, default=192, help='LR pixels per tile side (default 192)')
    ap.add_argument('--halo', type=int, default=None,
                    help="LR pixels of context per interior tile side (default: the generator's receptive halo -- exact result)")
    ap.add_argument('--feather', type=float, default=0.0, help='half-width of the seam cross-fade in LR pixels, 0 <= feather <= halo')
    ap.add_argument('--ensemble', type=int, default=1, choices=(1, 8), help='8: mean over the eight flips / transpositions')
    ap.add_argument('--batch', type=int, default=8, help='tiles per generator call (default 8)')
    ap.add_argument('--ema', action='store_true', help="use the averaged weights ('net_g_ema') of the checkpoint")
    ap.add_argument('--niqe', metavar='MODEL.npz', default=None,
                    help='also print the NIQE score of the output image under this model (tools/fit_niqe.py writes one)')
    a = ap.parse_args(argv)
    if a.tile < 1 or a.batch < 1:
        ap.error('--tile and --batch must be >= 1')
    if a.halo is not None and a.halo < 0:
        ap.error('--halo must be >= 0')
    if a.feather < 0 or (a.halo is not None and a.feather > a.halo):
        ap.error('--feather must lie in [0, halo]')
    return a


def arch_from_state(state):
    """The constructor arguments behind a generator state_dict, from its keys and shapes alone -> dict(n_blocks, n_features_block,
    n_features_last, list_scales, use_sn, input_channels, n_suffix); ``n_suffix`` GeneratorSuffix wrappers (keys under ``base.``)
    around a model_generator.Generator.  ValueError for another layout (e.g. the progressive generator's)."""
    prefix, n_suffix = '', 0
    while any(k.startswith(prefix + 'base.') for k in state):
        prefix, n_suffix = prefix + 'base.', n_suffix + 1
    core = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    first = core.get('first_layers.0.weight_orig')
    blocks = [int(m.group(1)) for m in (re.match(r'block_list\.(\d+)\.', k) for k in core) if m]
    stages = [int(m.group(1)) for m in (re.match(r'upscale\.(\d+)\.0\.', k) for k in core) if m]
    if first is None or not stages or not any(k.startswith('end.0.') for k in core):
        raise ValueError("not a model_generator.Generator state_dict: no 'first_layers.0.weight_orig', 'upscale.<i>.0.*' or "
                         "'end.0.*' among its keys")
    use_sn = 'upscale.0.0.weight_orig' in core
    up0 = core['upscale.0.0.weight_orig' if use_sn else 'upscale.0.0.weight']
    return dict(n_blocks=max(blocks) + 1 if blocks else 0, n_features_block=int(first.shape[0]), n_features_last=int(up0.shape[0]),
                list_scales=[2] * (max(stages) + 1), use_sn=use_sn, input_channels=int(first.shape[1]), n_suffix=n_suffix)


def build_generator(state):
    """a generator of the architecture ``arch_from_state`` reads, loaded tolerantly (strict=False; the base Generator prints the
    reference's coverage report when the checkpoint does not cover it)"""
    mg = _pkg('model_generator')
    arch = arch_from_state(state)
    net = mg.Generator(arch['n_blocks'], arch['n_features_block'], arch['n_features_last'], arch['list_scales'],
                       use_sn=arch['use_sn'], input_channels=arch['input_channels'])
    for _ in range(arch['n_suffix']):
        net = mg.GeneratorSuffix(net)
    net.load_state_dict(state, strict=False)
    return net


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    ckpt = torch.load(a.checkpoint, map_location='cpu')
    key = 'net_g_ema' if a.ema else 'net_g'
    if not isinstance(ckpt, dict) or key not in ckpt:
        sys.exit("%s holds no '%s' entry" % (a.checkpoint, key))
    if not torch.cuda.is_available():
        sys.exit('no MI355X device: this tool has no CPU path')
    net = build_generator(ckpt[key]).to('cuda')
    up = _pkg('upscale').Upscaler(net, tile=a.tile, halo=a.halo, feather=a.feather, ensemble=a.ensemble, batch=a.batch)
    img = torch.from_numpy(np.asarray(Image.open(a.input).convert('RGB')).copy()).to('cuda')
    sr = up(img)
    Image.fromarray(sr.cpu().numpy()).save(a.output)
    print('%s: %d x %d -> %s: %d x %d (x%d, %d tiles of %d, halo %d)'
          % (a.input, img.shape[1], img.shape[0], a.output, sr.shape[1], sr.shape[0], up.scale,
             up.ensemble * up.plan(img.shape[0], img.shape[1]).n, up.tile, up.halo))
    if a.niqe is not None:
        M = _pkg('metrics')
        model = M.NiqeModel.load(a.niqe).to('cuda')
        out = ((sr.permute(2, 0, 1)[None].float() - 127.5) / 127.5).contiguous()
        print('NIQE (model %s, block %d): %.4f' % (a.niqe, model.block, float(M.niqe(out, model))))


if __name__ == '__main__':
    main()
