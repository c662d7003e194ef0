#!/usr/bin/env python3
"""Fit a NIQE model from a folder of images: ``fit_niqe.py DIR OUT.npz [--block --sharpness --crop-border]``.

NIQE scores an image against a "pristine" model: the mean and the covariance of the 36 features over the sharp blocks of good
images (metrics.NiqeModel).  This tool fits one from the user's own images, as the paper does: every file of
DIR that Pillow reads is decoded on the host, converted to RGB and sent to the MI355X one at a time (the sizes may differ); the
features come from the kernels, the selection by sharpness and the moments from ``NiqeModel.fit``.  The result is written as an
``.npz`` with BasicSR's entry names.  Scores under different models are not comparable.  Argument handling needs no GPU.
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'single-image-super-resolution_amd'


def _pkg(sub):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + '.' + sub)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Fit a NIQE pristine model from a folder of images on the MI355X.')
    ap.add_argument('dir', help='folder of sharp, undistorted images (anything Pillow reads; converted to RGB)')
    ap.add_argument('output', help='the .npz to write (mu_pris_param, cov_pris_param, block)')
    ap.add_argument('--block', type=int, default=96, help='block side, even, 16 .. 96 (default 96)')
    ap.add_argument('--sharpness', type=float, default=0.75,
                    help="keep the blocks sharper than this share of their image's sharpest (default 0.75, the paper's rule)")
    ap.add_argument('--crop-border', type=int, default=0, help='pixels stripped from every side first (default 0)')
    a = ap.parse_args(argv)
    if a.block % 2 or not 16 <= a.block <= 96:
        ap.error('--block must be even and lie in 16 .. 96')
    if not 0.0 <= a.sharpness < 1.0:
        ap.error('--sharpness must lie in [0, 1)')
    if a.crop_border < 0:
        ap.error('--crop-border must be >= 0')
    return a


def images(folder, least, crop):
    """the decoded images of ``folder`` large enough for one block, as normalised [1, 3, H, W] fp32 device tensors, one at a time"""
    import numpy as np
    import torch
    from PIL import Image, UnidentifiedImageError
    for name in sorted(os.listdir(folder)):
        path = os.path.join(folder, name)
        if not os.path.isfile(path):
            continue
        try:
            rgb = np.asarray(Image.open(path).convert('RGB'))
        except (UnidentifiedImageError, OSError):
            print('skipped %s: not an image Pillow reads' % name)
            continue
        if min(rgb.shape[:2]) - 2 * crop < least:
            print('skipped %s: %d x %d leaves no %d x %d block' % (name, rgb.shape[1], rgb.shape[0], least, least))
            continue
        yield (torch.from_numpy(rgb.copy()).to('cuda').permute(2, 0, 1)[None].float() / 127.5 - 1.0).contiguous()


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not os.path.isdir(a.dir):
        sys.exit('%s is not a folder' % a.dir)
    if not torch.cuda.is_available():
        sys.exit('no MI355X device: this tool has no CPU path')
    M = _pkg('metrics')
    try:
        model = M.NiqeModel.fit(images(a.dir, a.block, a.crop_border), block=a.block, sharpness=a.sharpness, crop_border=a.crop_border)
    except ValueError as e:
        sys.exit(str(e))
    model.save(a.output)
    print('%s: block %d, sharpness %.2f -> %s' % (a.dir, a.block, a.sharpness, a.output))


if __name__ == '__main__':
    main()
