"""The conventions every device-side sampler shares (patches, degrade, jpeg, resize): the Python mirror of csrc/sisr_philox.h.

A draw is Philox4x32-10 under the key {seed low, seed high} on the counter {t low, t high, word 2, word 3}; word 3 says whose the
counter is (the table of DESIGN.md section 12): a patch-source sample's rank, ``tag | rank`` with rank < ``RANK_LIMIT``, or the
epoch permutation's ``TAG_PERM_KEY`` / ``TAG_PERM_BIT - round``.  Host code only: importing it touches no GPU.
"""
import numpy as np
import torch

RANK_LIMIT = 1 << 16
TAG_PERM_BIT, TAG_PERM_KEY = 0xFFFFFFFE, 0xFFFFFFFF
RANK_TAGS = dict(params=0xFE010000, noise=0xFE020000, quality=0xFE030000, mix_a=0xFE040000, mix_b=0xFE050000, mix_c=0xFE060000,
                 mix_final=0xFE070000, noise_grey=0xFE080000, mode=0xFE090000)                # the tags that are or-ed with a rank
TAG_QUALITY = RANK_TAGS['quality']
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy.  counter: [..., 4], key: [..., 2] words (broadcast against each other) ->
    [..., 4] uint32.  The host restatement of the generator in csrc/sisr_philox.h."""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2           # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def draw_words(seed, t, word2, word3):
    """draw_words of sisr_philox.h over ints or integer arrays that broadcast (``t``: a step or an epoch) -> [..., 4] uint32"""
    t, w2, w3 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (t, word2, word3)))
    return philox4x32_10(np.stack([t & _M32, t >> np.uint64(32), w2, w3], axis=-1), np.array([int(seed) & _M32, int(seed) >> 32], dtype=np.uint64))


def uniform24(words, dtype=np.float32):
    """draw_uniform of sisr_philox.h: u = ((r >> 8) + 0.5) 2^-24 in (0, 1], in fp32 as the device computes it (or float64)"""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)


def check_seed(seed, who):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError('%s: seed must be in [0, 2^64), got %d' % (who, seed))
    return seed


def check_seed_rank(seed, rank, who):
    seed, rank = check_seed(seed, who), int(rank)
    if not 0 <= rank < RANK_LIMIT:
        raise ValueError('%s: rank must be in [0, %d), got %d' % (who, RANK_LIMIT, rank))
    return seed, rank


def step_tensor(step, device=None, strict=None):
    """the step a kernel reads: a 0-dim int64 device tensor is used where it lies (a captured call follows it); a host int or
    None (0) becomes one on ``device`` -- or, with ``strict`` = the caller's name, is refused"""
    if isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.int64 and step.numel() == 1:
        return step
    if strict is not None:
        raise ValueError('%s: the step is a 0-dim int64 device tensor' % strict)
    return torch.full((), 0 if step is None else int(step), dtype=torch.int64, device=device)


class DrawStream:
    """a sampler object's ``seed`` and ``rank`` (key and stream of its draws) and ``step``, the 0-dim int64 device tensor of draws made"""

    def _init_stream(self, seed, rank, device):
        who = type(self).__name__
        self.seed, self.rank = check_seed_rank(seed, rank, who)
        dev = torch.device('cuda' if device is None else device)
        if dev.type != 'cuda':
            raise RuntimeError('%s: the draws live on the MI355X (got device %s); there is no CPU fallback' % (who, dev))
        self.step = torch.zeros((), dtype=torch.int64, device=dev)

    def state_dict(self):
        return dict(seed=self.seed, rank=self.rank, step=self.step.clone())

    def load_state_dict(self, state):
        """copies the count INTO the existing tensor (a captured draw points at it)"""
        seed, rank = check_seed_rank(state['seed'], state['rank'], type(self).__name__ + '.load_state_dict')
        self.step.copy_(torch.as_tensor(state['step'], dtype=torch.int64).reshape(()))
        self.seed, self.rank = seed, rank
