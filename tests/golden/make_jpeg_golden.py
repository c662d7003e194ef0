"""Writes tests/golden/jpeg_pillow.npz: what a real JPEG codec (Pillow / libjpeg) does, recorded once so that no test imports PIL.

  python tests/golden/make_jpeg_golden.py

  qualities          the qualities of the recorded tables
  tables             [len(qualities), 2, 8, 8] uint8: the decoder's luma and chroma quantisation tables, row-major (checked here
                     against Annex K at quality 50, where libjpeg's scale factor is 1)
  image              [3, 40, 52] uint8: a smooth sinusoid per channel plus N(0, 0.1) noise (seed 0), clipped
  roundtrip_q        the qualities of the recorded round trips
  roundtrip          [len(roundtrip_q), 3, 40, 52] uint8: `image` encoded at 4:4:4 and decoded
"""
import io
import os

import numpy as np
from PIL import Image

QUALITIES = (1, 10, 25, 49, 50, 75, 90, 95, 100)
ROUNDTRIP_Q = (10, 50, 90)
ANNEX_K_LUMA_ROW0 = [16, 11, 10, 16, 24, 40, 51, 61]
ANNEX_K_CHROMA_ROW0 = [17, 18, 24, 47, 99, 99, 99, 99]


def fixture_image():
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(40.0), np.arange(52.0), indexing='ij')
    chans = [0.5 + 0.4 * np.sin(0.23 * xx + 0.11 * yy), 0.5 + 0.4 * np.sin(0.07 * xx - 0.19 * yy + 1.0),
             0.5 + 0.4 * np.cos(0.13 * xx + 0.17 * yy + 2.0)]
    img = np.stack(chans) + rng.normal(0.0, 0.1, size=(3, 40, 52))
    return np.round(np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8)


def encode_decode(img_chw, q):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img_chw.transpose(1, 2, 0))).save(buf, 'JPEG', quality=q, subsampling=0)
    im = Image.open(io.BytesIO(buf.getvalue()))
    tables = np.array([list(im.quantization[0]), list(im.quantization[1])], dtype=np.uint8).reshape(2, 8, 8)
    return tables, np.asarray(im.convert('RGB')).transpose(2, 0, 1).copy()


def main():
    img = fixture_image()
    tables = np.stack([encode_decode(img, q)[0] for q in QUALITIES])
    i50 = QUALITIES.index(50)
    assert tables[i50, 0, 0].tolist() == ANNEX_K_LUMA_ROW0 and tables[i50, 1, 0].tolist() == ANNEX_K_CHROMA_ROW0, 'tables are not row-major'
    trips = np.stack([encode_decode(img, q)[1] for q in ROUNDTRIP_Q])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_pillow.npz')
    np.savez_compressed(out, qualities=np.array(QUALITIES, np.int32), tables=tables, image=img,
                        roundtrip_q=np.array(ROUNDTRIP_Q, np.int32), roundtrip=trips)
    print('wrote %s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
