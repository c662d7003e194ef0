"""The definition, the cases, the inputs, the float64 references and the bounds shared by test_contextual_cpu.py and
test_gpu_contextual.py (a plain module, not a conftest): the contextual loss of Mechrez, Talmi and Zelnik-Manor (ECCV 2018) in its
cosine form.  Everything here is float64 on the CPU unless a dtype is passed.

A feature tensor is (B, total) in the layout of MaskedVGG.forward: tap l is columns [off_l, off_l + C_l P_l) of every row in NCHW
order, P_l = H_l W_l; X[n], Y[n] the C x P slices of fa (the generator side) and fb (the target, a constant), column i the point x_i:
  mu = mean of Y over batch and points (a C-vector)     x^_i = (x_i - mu) / max(|x_i - mu|, 1e-12),  y^_j likewise
  S_ij = x^_i . y^_j    d = 1 - S    m_i = min_j d_ij    w_ij = exp((1 - d_ij / (m_i + 1e-5)) / h)    Z_i = sum_j w_ij    CX_ij = w_ij / Z_i
  c_j = max_i CX_ij    CX[n] = mean_j c_j    T_l = mean_n -log(CX[n] + 1e-5)    loss = weight sum_l w_l T_l
Ties of the min (j*) and of the max (i*) take the lowest index."""
import functools
import importlib
import math

import torch

F64 = torch.float64
U = 2.0 ** -24                      # one fp32 rounding, relative
EPS = 1e-5
TINY = 1e-12
SLACK = 1.01                        # the second-order terms of the first-order bounds below
FLOOR = 2.0 ** -149                 # the smallest fp32 step: results that underflow have no relative bound


def pkg(sub=None):
    return importlib.import_module('single-image-super-resolution_amd' + ('.' + sub if sub else ''))


# (B, shapes, layer weights, relu): the smallest shapes at which the kernels can still go wrong.  No C < 3: with C = 2 the unit vectors tie
CASES = [
    (2, ((5, 1, 7),), (1.0,), False),
    (3, ((48, 5, 7),), (1.0,), False),                               # C no multiple of 32, P = 35
    (2, ((130, 3, 11),), (1.0,), False),                             # C two past four tiles of 32, P = 33: one past a tile
    (1, ((32, 1, 1),), (1.0,), False),                               # P = 1
    (2, ((64, 12, 12),), (1.0,), True),                              # P = 144: three tiles of 64 with a ragged one, ReLU-ed features
    (1, ((256, 24, 24),), (1.0,), False),                            # conv3_4 at HR 96^2: S is 1.3 MB, three elements a thread in the row pass
    (2, ((5, 3, 3), (24, 6, 10), (40, 3, 5)), (0.75, 1.0, 1.25), False),      # the second tap starts at column 45: 4-byte alignment only
    (17, ((8, 2, 2),), (1.0,), False),                               # B above 16
]
SMALL = [c for c in CASES if max(h * w for _, h, w in c[1]) <= 144]  # the end-to-end comparison runs on these
KINDS = ('uniform', 'correlated')
BAND = 0.5


def case_id(case):
    return 'B%d-%s%s' % (case[0], 'x'.join('%d.%d.%d' % s for s in case[1]), '-relu' if case[3] else '')


def total_of(shapes):
    return sum(c * h * w for c, h, w in shapes)


def split(feat, shapes):
    """-> the taps of a (B, total) tensor as (B, C, P) views"""
    out, off = [], 0
    for c, h, w in shapes:
        out.append(feat[:, off:off + c * h * w].reshape(feat.shape[0], c, h * w))
        off += c * h * w
    return out


@functools.lru_cache(maxsize=None)
def inputs(b, shapes, relu=False, kind='uniform', seed=1):
    """-> (fa, fb) fp32 (B, total); never modified.  uniform: independent values in [-1, 1) (relu: the negative ones zeroed);
    correlated: fa = fb + 0.5 noise, so that m_i is small and the loss is not saturated"""
    gen = torch.Generator().manual_seed(300 + seed)
    r = [2 * torch.rand((b, total_of(shapes)), generator=gen, dtype=F64) - 1 for _ in range(2)]
    fb = r[1].clamp_min(0) if relu else r[1]
    fa = r[0] if kind == 'uniform' else fb + 0.5 * r[0]
    fa = fa.clamp_min(0) if relu else fa
    return fa.to(torch.float32), fb.to(torch.float32)


# ---- the common PyTorch text of the cosine form, in the dtype of its inputs ----------------------------------------------------------
def composition(fa, fb, shapes, layer_weights, band_width=BAND, weight=1.0):
    """y-mean centring, F.normalize, bmm, min over the target axis, max over the source axis -> the scalar.  fb is detached"""
    loss = 0
    for x, y, wl in zip(split(fa, shapes), split(fb.detach(), shapes), layer_weights):
        mu = y.mean(dim=(0, 2), keepdim=True)
        xh = torch.nn.functional.normalize(x - mu, p=2, dim=1)
        yh = torch.nn.functional.normalize(y - mu, p=2, dim=1)
        d = 1 - torch.bmm(xh.transpose(1, 2), yh)                    # (B, P_i, P_j)
        dmin = d.min(dim=2, keepdim=True)[0]
        w = torch.exp((1 - d / (dmin + EPS)) / band_width)
        cx = w / w.sum(dim=2, keepdim=True)
        cxn = cx.max(dim=1)[0].mean(dim=1)
        loss = loss + wl * (-torch.log(cxn + EPS)).mean()
    return weight * loss


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------
def first_arg(t, value, dim):
    """the LOWEST index along dim at which t equals value (broadcast)"""
    return (t == value).to(torch.int8).argmax(dim)                  # argmax returns the first maximal value


def normalise64(x, mu):
    """x (B, C, P), mu (C) -> (x^, |x - mu|) with the norm (B, 1, P)"""
    xc = x.to(F64) - mu.to(F64).view(1, -1, 1)
    nrm = xc.pow(2).sum(1, keepdim=True).sqrt()
    return xc / nrm.clamp_min(TINY), nrm


def sim64(fa, fb, shapes):
    """-> per tap (S (B, P, P), mu (C)) from the raw inputs"""
    out = []
    for x, y in zip(split(fa.to(F64), shapes), split(fb.to(F64), shapes)):
        mu = y.mean(dim=(0, 2))
        out.append((torch.bmm(normalise64(x, mu)[0].transpose(1, 2), normalise64(y, mu)[0]), mu))
    return out


def rows64(d, band_width):
    """d (B, P, P) float64 -> dict: m, jstar, den, arg, w, Z, CX"""
    m = d.min(dim=2)[0]
    jstar = first_arg(d, m.unsqueeze(2), 2)
    den = m + EPS
    arg = (1 - d / den.unsqueeze(2)) / band_width
    w = arg.exp()
    Z = w.sum(2)
    return dict(d=d, m=m, jstar=jstar, den=den, arg=arg, w=w, Z=Z, CX=w / Z.unsqueeze(2))


def cols64(CX):
    """-> c (B, P), istar (B, P), CX[n] (B)"""
    c = CX.max(dim=1)[0]
    return c, first_arg(CX, c.unsqueeze(1), 1), c.mean(1)


def d_of(S):
    """d = 1 - S in float64; from an FP32 S (the device's) the fp32 subtraction is repeated first, so that d has the device's bits"""
    return (1 - S).to(F64)


def forward64(fa, fb, shapes, layer_weights, band_width=BAND, weight=1.0, sims=None):
    """-> (loss, terms [n_taps], cx [n_taps, B], per-tap dicts); `sims`: per-tap fp32 S that replace the restatement's own"""
    taps, terms, cxs = [], [], []
    own = sim64(fa, fb, shapes) if sims is None else None
    for l in range(len(shapes)):
        r = rows64(d_of(own[l][0] if sims is None else sims[l]), band_width)
        r['c'], r['istar'], r['cxn'] = cols64(r['CX'])
        taps.append(r)
        cxs.append(r['cxn'])
        terms.append((-torch.log(r['cxn'] + EPS)).mean())
    terms = torch.stack(terms)
    return weight * (torch.tensor(layer_weights, dtype=F64) * terms).sum(), terms, torch.stack(cxs), taps


def grad64(x, y, mu, r, istar, jstar, cxn, coeff, band_width=BAND, Z=None, na=None, nb=None):
    """The gradient formulas for one tap -> (dloss / dx (B, C, P), the pieces as a dict).  x, y (B, C, P); r: rows64 of the tap's d;
    istar, jstar (B, P); cxn (B); coeff = g weight w_l.  Z, na, nb: the device's tables in place of the restatement's own.
      gamma_n = -coeff / (B (CX[n] + 1e-5))        G_ij = gamma_n / P where i = i*(j), else 0        r_i = sum_j G_ij CX_ij
      E_ij = -CX_ij (G_ij - r_i) / h        q_i = sum_j E_ij d_ij        dloss / dd_ij = E_ij / (m_i + 1e-5) - [j = j*(i)] q_i / (m_i + 1e-5)^2
      T = -dloss / dd        dloss / dx^ = Y^ T^T        dloss / dx_i = (v - x^_i (x^_i . v)) / |x_i - mu|, 0 where the norm is below 1e-12"""
    b, _, p = x.shape
    d, den = r['d'], r['den']
    CX = r['CX'] if Z is None else r['w'] / Z.to(F64).unsqueeze(2)
    gp = -coeff / (b * (cxn.to(F64) + EPS)) / p                      # (B)
    top = torch.zeros_like(CX).scatter_(1, istar.long().unsqueeze(1), 1.0)        # [n, i*(j), j] = 1
    G = top * gp.view(b, 1, 1)
    ri = (G * CX).sum(2)
    E = -CX * (G - ri.unsqueeze(2)) / band_width
    q = (E * d).sum(2)
    dd = E / den.unsqueeze(2)
    pick = torch.zeros_like(CX).scatter_(2, jstar.long().unsqueeze(2), 1.0)
    dd = dd - pick * (q / den.pow(2)).unsqueeze(2)
    xh, xn = normalise64(x, mu)
    yh, yn = normalise64(y, mu)
    if na is not None:
        xn = na.to(F64).unsqueeze(1)
        xh = (x.to(F64) - mu.to(F64).view(1, -1, 1)) / xn.clamp_min(TINY)
    yc = y.to(F64) - mu.to(F64).view(1, -1, 1)
    inv_b = 1 / (yn if nb is None else nb.to(F64).unsqueeze(1)).clamp_min(TINY)      # (B, 1, P_j)
    Tp = -dd * inv_b                                                 # T_ij / |y_j - mu|
    v = torch.einsum('ncj,nij->nci', yc, Tp)
    dx = (v - xh * (xh * v).sum(1, keepdim=True)) / xn.clamp_min(TINY)
    dx = torch.where(xn < TINY, torch.zeros_like(dx), dx)
    return dx, dict(CX=CX, gp=gp, top=top, G=G, r=ri, E=E, q=q, dd=dd, pick=pick, Tp=Tp, v=v, xh=xh, xn=xn, yc=yc, inv_b=inv_b)


def loss_grad64(fa, fb, shapes, layer_weights, band_width=BAND, weight=1.0, g=1.0):
    """the restated gradient of the whole loss from the raw inputs -> (B, total)"""
    _, _, _, taps = forward64(fa, fb, shapes, layer_weights, band_width, weight)
    out = []
    for x, y, (_, mu), r, wl in zip(split(fa, shapes), split(fb, shapes), sim64(fa, fb, shapes), taps, layer_weights):
        out.append(grad64(x, y, mu, r, r['istar'], r['jstar'], r['cxn'], g * weight * wl, band_width)[0].reshape(x.shape[0], -1))
    return torch.cat(out, 1)


def margins64(taps):
    """the smallest margins of the float64 reference's discrete choices: min_i (d_(2) - d_(1)) over the rows and the smallest relative
    gap of the two largest CX_.j over the columns; inf where a row or a column has one element"""
    gap_d, gap_c = math.inf, math.inf
    for r in taps:
        if r['d'].shape[2] > 1:
            two = r['d'].topk(2, dim=2, largest=False)[0]
            gap_d = min(gap_d, float((two[..., 1] - two[..., 0]).min()))
            top = r['CX'].topk(2, dim=1)[0]
            gap_c = min(gap_c, float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
    return gap_d, gap_c


# ---- the bounds: derived from the arithmetic, never from a kernel's output ---------------------------------------------------------------
def sim_bound(fa, fb, shapes):
    """|S_dev - S64| element by element -> per tap (B, P, P).  The device forms mu in double and rounds it once, centres in fp32
    (x - mu: one rounding), so a centred element is off by at most e = u (|mu_c| + |x_c - mu_c|); normalising a vector that is off by e
    moves the unit vector by at most 2 |e| / |x - mu| (in the 2-norm), and a unit vector on the other side turns that into the same
    change of the dot product.  The chain itself: C fma roundings in channel order on v_mfma_f32_32x32x2_f32, then (acc * ia) * ib with
    ia = fl(1 / fl(sqrt(sum of squares in double))): two roundings for each reciprocal norm and two for the two products, so
    k = 6:  |S_dev - S64| <= (C + 6) u sum_c |x^_ic| |y^_jc| + dx_i + dy_j + dx_i dy_j"""
    out = []
    for x, y in zip(split(fa.to(F64), shapes), split(fb.to(F64), shapes)):
        mu = y.mean(dim=(0, 2))
        c = x.shape[1]

        def moved(t):
            tc = t - mu.view(1, -1, 1)
            e = U * (mu.abs().view(1, -1, 1) + tc.abs())
            return 2 * SLACK * e.pow(2).sum(1).sqrt() / tc.pow(2).sum(1).sqrt()      # (B, P)
        dx, dy = moved(x).unsqueeze(2), moved(y).unsqueeze(1)
        chain = (c + 6) * U * SLACK * torch.bmm(normalise64(x, mu)[0].abs().transpose(1, 2), normalise64(y, mu)[0].abs())
        out.append(chain + dx + dy + dx * dy)
    return out


def row_bounds(r, band_width):
    """The roundings behind S, against rows64 / cols64 of the device's own S -> dict of bounds.
      den_dev = fl(m + fl(1e-5)): 2 u.  dt = fl(d / den): 3 u in all.  a = fl(fl(1 - dt) fl(1 / h)):
      |da| <= u (3 |dt| / h + 3 |a|) <= u (6 |a| + 3 / h).  expf within one ulp (2 u relative):  rho_ij = expm1(da) + 2 u, and an
      underflowing w has the absolute floor 2^-149.  Z: the sum in double (its own error is 1e-16 of Z), one rounding to fp32.
      CX = fl(w / Z): rho_ij + eZ_i / Z_i + u.  c_j = max_i: |max a - max b| <= max |a - b|.  CX[n]: the mean in double, one rounding."""
    rho = torch.expm1(U * (6 * r['arg'].abs() + 3 / band_width)) + 2 * U
    ew = r['w'] * rho + FLOOR
    eZ = SLACK * (ew.sum(2) + U * r['Z'])
    eCX = SLACK * r['CX'] * (rho + (eZ / r['Z']).unsqueeze(2) + U) + FLOOR
    ec = eCX.max(dim=1)[0]
    ecxn = SLACK * (ec.mean(1) + U * r['cxn'])
    return dict(rho=rho, eZ=eZ, eCX=eCX, ec=ec, ecxn=ecxn)


def term_bound(cxn, ecxn):
    """|T_dev - T64| for one tap: -log(CX[n] + 1e-5) moves by at most e / (CX[n] + 1e-5 - e); the mean in double, one rounding"""
    t = (-torch.log(cxn + EPS)).mean()
    return float(SLACK * ((ecxn / (cxn + EPS - ecxn)).mean() + U * t.abs()))


def grad_bound(r, pc, band_width, rho):
    """|dfa_dev - grad64| element by element for one tap, grad64 evaluated on the device's own S and tables (pc: its pieces) -> (B, C, P).
    The device recomputes CX_ij = fl(w / Z) with the forward's bits: relative rho' = rho + u against w64 / Z_dev.  gamma / P is formed in
    double and rounded once (2 u with the rounded CX[n] + 1e-5).  r_i = fl(gp fl(sum in double)): er_i = |gp| sum_top CX rho' + 4 u |r_i|.
    d(G - r) <= 2 u |G| + er + u |G - r|.  E = fl(fl(-CX (G - r)) fl(1 / h)): dE <= |E| (rho' + 3 u) + CX d(G - r) / h.
    q_i = fl(sum in double of E d): dq <= sum_j dE |d| + u |q|.  den: 2 u.  dd = fl(fl(E / den) - fl(q / fl(den^2))):
    d(E / den) <= (dE + 3 u |E|) / den, dpick <= (dq + 6 u |q|) / den^2, one rounding of the difference; T' = fl(-dd fl(1 / nb)): 2 u more.
    The product Y^ T'^T: a chain of P fma roundings in point order over the centred y (one rounding each): (P + 2) u (|T'| |yc|) + eT |yc|.
    The projection: x^ = fl(fl(x - mu) ia) (3 u), the dot in double rounded once, v - x^ dot, the last product: 8 u on every term."""
    h = band_width
    rp = rho + U
    CX, G, E, d, den = pc['CX'], pc['G'], pc['E'], r['d'], r['den'].unsqueeze(2)
    gp = pc['gp'].abs().view(-1, 1)
    er = gp * (pc['top'] * CX * rp).sum(2) + 4 * U * pc['r'].abs()
    gr = G - pc['r'].unsqueeze(2)
    dgr = 2 * U * G.abs() + er.unsqueeze(2) + U * gr.abs()
    dE = E.abs() * (rp + 3 * U) + CX * dgr / h
    dq = (dE * d.abs()).sum(2) + U * pc['q'].abs()
    dEd = (dE + 3 * U * E.abs()) / den
    dpick = pc['pick'] * ((dq + 6 * U * pc['q'].abs()) / r['den'].pow(2)).unsqueeze(2)
    eT = SLACK * (dEd + dpick + 3 * U * pc['dd'].abs()) * pc['inv_b'] + FLOOR
    p = CX.shape[2]
    yabs = pc['yc'].abs()
    ev = SLACK * ((p + 2) * U * torch.einsum('ncj,nij->nci', yabs, pc['Tp'].abs()) + torch.einsum('ncj,nij->nci', yabs, eT))
    xh, v, xn = pc['xh'].abs(), pc['v'], pc['xn'].clamp_min(TINY)
    dot_abs = (xh * v.abs()).sum(1, keepdim=True)
    eo = (ev + xh * (xh * ev).sum(1, keepdim=True) + 8 * U * (v.abs() + xh * dot_abs)) / xn
    return SLACK * eo + FLOOR
