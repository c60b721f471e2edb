"""float64 references, case lists, wrong variants and derived bounds of the three kernels of csrc/vad.hip — vad_frontend_batch_kernel,
vad_lstm_batch_kernel, vad_out_kernel — in the kernels' output layouts, restated from oracle/silero_vad.py. Host only (numpy); the
run_* functions at the end call the wlx_vad_debug_* hooks and are used by tests/test_gpu_vad_kernels.py. tests/test_vad_kernel_ref.py
shows on these references alone that every wrong variant leaves its bound on a named case and that a float32 run of the restatement
stays inside every bound, so that a bound is a statement about float32 arithmetic and not about one kernel.

LAYOUTS. gx [windows][512]: row w = W_ih f_w + b_ih + b_hh, gate order i, f, g, o (f_w the 128 features of window w). hs [windows][512]:
row w = [unit j][4 copies of h_j]; the output kernel reads copy 0. probs [windows].

THE BOUNDS are first-order forward error bounds evaluated next to the reference, with u = 2^-24 (the relative error of one float32
rounding) and every result multiplied by SLACK = 1.05 (the second-order terms) plus FLOOR = 2^-125 (a result the instructions may flush).
* A dot product. Whatever the order of the additions, sum_k w_k x_k computed with fused multiply-adds is off by at most
  D u sum |w_k||x_k| where D is the largest number of roundings one term passes through; D <= K for K terms, and "K + small" below is K
  plus the roundings of the bias additions. Inputs that carry errors d_k of their own add sum |w_k| d_k.
* Front end. The samples are exact. STFT: K = 256 (+2: the Nyquist bin's sixteen partial sums are added in a second pass).
  Magnitude: sqrt(re^2 + im^2) is 1-Lipschitz in (re, im), so the input errors contribute sqrt(d_re^2 + d_im^2); the two squares, their
  sum and the root: the radicand is off by 2u relative, the root halves that, the root instruction adds SQRT_ULPS ulps = 2u SQRT_ULPS:
  (1 + 2 SQRT_ULPS) u mag. Convolutions: K = 3 Cin + 1 (bias). Gates: K = 128 + 2 (the folded bias b_ih + b_hh is itself rounded
  once, and added once). Through the layers the errors are carried by the SIGNED linear maps of the reference point (ReLU masks times
  weights), the absolute value taken of the whole product (_fe_bound_one): factor by factor the bound would grow 30-fold per layer and
  reach 100 on rows of size 5. ReLU is 1-Lipschitz: a unit within its own bound of the kink passes that bound on and nothing else.
* Recurrence, one step. The pre-activation of gate row r is gx_r + sum_k W_hh[r][k] h_k: a lane's 32 terms run through two chains of
  16 fused multiply-adds that are added (1), the four lanes of a quad are added in two steps (2), gx is added last (1):
  LSTM_DOT_U = 20. sigmoid(x) = rcp(1 + E(-x)) with E = __expf: E carries eps_E(x) = 2u EXP2_ULPS + |x| (2u + KAPPA) (derived in
  tests/prob_kernel_ref.py: instruction, argument scaling, the constant log2 e), which moves s = sigmoid(x) by s (1 - s) eps_E; the
  addition and the reciprocal (RCP_ULPS ulps) move it by s (1 + 2 RCP_ULPS) u. The candidate gate is 2 sigmoid(2x) - 1: twice that
  at 2x, and u |g| for the subtraction. c' = f c + i g: every term passes two roundings at most, fused or not: 2u (|f c| + |i g|).
  tanh(c') = 1 - 2 r, r = rcp(1 + E(2c')): r is off by r (sigmoid(2c') eps_E(2c') + (1 + 2 RCP_ULPS) u), and the subtraction by
  u |tanh|: where c' is small the result cancels and this ABSOLUTE error of a few u stays, which is what the bound then allows.
  h = o tanh(c'): u |h|. Where E overflows to inf or flushes to 0 the gate is exactly 0 or 1 and the true value is within FLOOR of it.
* Recurrence, T steps. With z_t = (h_t, c_t), the computed trajectory satisfies, to first order, dz_t = J_t dz_{t-1} + E_t r_t, J_t the
  Jacobian of one step at the REFERENCE point (the derivatives s (1 - s), 1 - g^2, 1 - tanh^2 of the gate non-linearities there), r_t the
  step's own errors (|r_t| <= rho_t, the one-step figures above: rho_c for c', rho_h for what h adds) and E_t how they enter
  (r_c reaches h_t through o (1 - tanh^2)). So |dh_t| <= sum_{s <= t} |J_t ... J_{s+1} E_s| rho_s, the absolute value taken AFTER the
  matrix product: taking it factor by factor would let the bound grow like (|W_hh| row sums)^t, which is 10^39 at t = 65. The
  reference carries the products Q_{t,s} along (lstm_ref).
* Output layer. A lane's two products and sum (2), the six-deep wave sum (6), the bias (1): OUT_DOT_U = 9; the sigmoid as above with
  the division taken as DIV_ULPS ulps. The kernel calls the precise expf here; eps_E, the figure of the fast form, is at least as
  large and is used for it.
ASSUMED (no document installed with the toolchain states them): EXP2_ULPS, RCP_ULPS, SQRT_ULPS, DIV_ULPS = 1 ulp each.
No constant here was fitted to what a kernel returned.

THE SECOND WEIGHT FAMILY. "scaled" is the base family with lstm_w_hh multiplied by WHH_SCALE, so that the recurrent term alone
saturates gates (|W_hh h| reaches several units per unit of |h|). The factor was chosen on the CPU: test_vad_kernel_ref.py admits it
only while the first-order bound of the T = 65 cases still rejects every wrong variant of the recurrence; see WHH_SCALE below for the
value and the resulting bound-to-signal ratio."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import silero_vad as sv

U = 2.0 ** -24
EXP2_ULPS = 1.0                                   # ASSUMED accuracy of v_exp_f32, in ulps
RCP_ULPS = 1.0                                    # ASSUMED accuracy of v_rcp_f32
SQRT_ULPS = 1.0                                   # ASSUMED accuracy of sqrtf as compiled
DIV_ULPS = 1.0                                    # ASSUMED accuracy of the float32 division as compiled
LOG2E_F32 = float(np.float32(1.4426950408889634))
KAPPA = abs(LOG2E_F32 - math.log2(math.e)) / math.log2(math.e)
FLOOR = 2.0 ** -125
SLACK = 1.05
GUARD = 64                                        # WLX_DEBUG_GUARD
FILL = 1000.0                                     # outputs are pre-filled with +-FILL
H = 128
LSTM_DOT_U = 16 + 1 + 2 + 1
OUT_DOT_U = 2 + 6 + 1
SEED = 5
# lstm_w_hh of the "scaled" family = WHH_SCALE x the base family's. Chosen on the CPU among 2, 3, 4 and 8 as the largest factor that
# tests/test_vad_kernel_ref.py test_whh_scale_is_admitted admits: at the LAST step of the T = 65 Gaussian cases the gate-order and
# quarter variants still leave the bound, and the largest bound of the family's T = 65 cases stays below BOUND_TO_SIGNAL_MAX of the
# signal scale 1 (h lies in (-1, 1)). Measured on the CPU: factor 2: 2.1e-4; 3: 4.2e-3 (the variants leave the bound 5e3-fold at the
# last step); 4: 0.34, no statement any more; 8: the recurrence is chaotic, the float32 run of the restatement itself is 3.6 bounds
# away from the float64 one.
WHH_SCALE = 3.0
BOUND_TO_SIGNAL_MAX = 1e-2


def eps_exp(x):
    return 2 * U * EXP2_ULPS + np.abs(x) * (2 * U + KAPPA)


def _sig(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


@functools.lru_cache(maxsize=None)
def weights(family="base"):
    """the seeded stand-in weights of the tests: oracle.silero_vad.random_weights with a non-zero output bias; "scaled": W_hh x WHH_SCALE"""
    w = sv.random_weights(SEED)
    w["out_b"] = np.asarray([0.25], np.float32)
    if family == "scaled":
        w["lstm_w_hh"] = (w["lstm_w_hh"] * np.float32(WHH_SCALE)).astype(np.float32)
    else:
        assert family == "base"
    return w


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (> 1: outside the bound); inf when anything is not finite"""
    got, ref, bound = (np.asarray(a, np.float64).ravel() for a in (got, ref, bound))
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max()) if got.size else 0.0


# ------------------------------------------------------------------ front end
FE_WRONGS = ("no_b_hh", "tail_off_by_one", "nyquist_dropped", "conv3_tap0", "conv2_shifted", "context_zero", "context_from_neighbour")


def windows_of(n, extra):
    return (int(n) + 511) // 512 + int(extra)


def fe_frames(x, extra, before=None, variant=None):
    """one item's [T][576] frames: 64 samples of context (zeros at the first window, whatever lies in front of the item) + 512 samples,
    zeros past the n samples. `before`: the 64 samples in front of the item in the packed buffer (the "context_from_neighbour" variant)."""
    x = np.asarray(x, np.float32)
    T = windows_of(x.shape[0], extra)
    p = np.zeros(T * 512, np.float32)
    p[:x.shape[0]] = x
    p = p.reshape(T, 512)
    ctx = np.zeros((T, 64), np.float32)
    if variant != "context_zero":
        ctx[1:] = p[:-1, -64:]
    if variant == "context_from_neighbour" and before is not None and T:
        ctx[0] = before
    return np.concatenate([ctx, p], axis=1)


def _conv(x, w, b, stride, shift=0):
    """conv1d k3, zero pad 1 (+ `shift` positions to the right: the "conv2_shifted" variant); x [N][Cin][L]"""
    n, _cin, length = x.shape
    lout = (length + 2 - 3) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1 + shift)))
    out = np.empty((n, w.shape[0], lout), x.dtype)
    for t in range(lout):
        a = t * stride + shift
        out[:, :, t] = np.einsum("ncj,ocj->no", xp[:, :, a:a + 3], w) + b
    return out


_FE_LEN = (4, 4, 2, 1, 1)          # positions of mag and of the four convolutions' outputs


def _fe_dense(w):
    """the four convolutions and the gate projection as dense matrices over (channel, position), with their biases and term counts:
    layer k maps the post-activation of layer k - 1 (layer 0: the magnitudes [129][4]) to its pre-activation"""
    key = id(w)
    if key in _fe_dense.cache:
        return _fe_dense.cache[key]
    out = []
    for i, (cin, cout, stride) in enumerate(sv.ENC_CHANNELS):
        lin, lout = _FE_LEN[i], _FE_LEN[i + 1]
        wi = w[f"enc{i}_w"].astype(np.float64)
        m = np.zeros((cout, lout, cin, lin))
        for t in range(lout):
            for j in range(3):
                p = t * stride + j - 1
                if 0 <= p < lin:
                    m[:, t, :, p] = wi[:, :, j]
        out.append((m.reshape(cout * lout, cin * lin), np.repeat(w[f"enc{i}_b"].astype(np.float64), lout), 3 * cin + 1))
    bias = w["lstm_b_ih"].astype(np.float64) + w["lstm_b_hh"].astype(np.float64)
    out.append((w["lstm_w_ih"].astype(np.float64), bias, 128 + 2))
    _fe_dense.cache[key] = out
    return out


_fe_dense.cache = {}


def _fe_bound_one(layers, mag, dmag):
    """the bound of one window's gx row: mag, dmag [129][4]. The error of layer k's pre-activation is, to first order,
    sum_l (W_k A_{k-1} ... A_{l+1}) s_l + its own rounding, A = diag(ReLU mask) W and s_l the errors that ENTER behind layer l
    (the magnitudes' for l = 0, the rounding of a live unit); the absolute value is taken of the whole product. A unit whose
    pre-activation lies within its own bound of the kink may come out on either side: its mask is uncertain, so nothing is carried
    through it and its whole bound enters as a new error behind it (the ReLU is 1-Lipschitz)."""
    post = mag.ravel()
    srcs = [dmag.ravel()]           # s_l
    G = [None]                      # G[l]: post of the current layer <- source l (None: the identity)
    for k, (Wk, bk, terms) in enumerate(layers):
        X = [Wk if g is None else Wk @ g for g in G]
        pre = Wk @ post + bk
        rho = terms * U * (np.abs(Wk) @ np.abs(post) + np.abs(bk))
        b = SLACK * (sum(np.abs(x) @ s for x, s in zip(X, srcs)) + rho) + FLOOR
        if k == len(layers) - 1:
            return b
        kink = np.abs(pre) <= b
        live = (pre > 0) & ~kink
        G = [x * live[:, None] for x in X] + [None]
        srcs.append(np.where(kink, b, live * rho))
        post = np.maximum(pre, 0)


def fe_rows(w, frames, dtype=np.float64, variant=None):
    """[N][576] frames -> gx [N][512] and its bound (None unless dtype is float64 and no variant is asked for)"""
    want_bound = dtype == np.float64 and variant is None
    x = np.asarray(frames, dtype)
    tail = x[:, -3: -3 - 64: -1] if variant == "tail_off_by_one" else x[:, -2: -2 - 64: -1]
    x = np.concatenate([x, tail], axis=1)                                   # [N][640]
    basis = w["stft_basis"].astype(dtype)
    seg = np.stack([x[:, t * 128: t * 128 + 256] for t in range(4)], axis=1)   # [N][4][256]
    spec = seg @ basis.T
    re, im = spec[..., :129], spec[..., 129:]
    mag = np.sqrt(re * re + im * im).transpose(0, 2, 1)                     # [N][129][4]
    if variant == "nyquist_dropped":
        mag = mag.copy()
        mag[:, 128, :] = 0
    y = mag
    for i, (_cin, _cout, stride) in enumerate(sv.ENC_CHANNELS):
        wi = w[f"enc{i}_w"].astype(dtype)
        if variant == "conv3_tap0" and i == 2:                               # taps 0, 1 where taps 1, 2 belong
            wi = np.concatenate([np.zeros_like(wi[:, :, :1]), wi[:, :, :2]], axis=2)
        y = np.maximum(_conv(y, wi, w[f"enc{i}_b"].astype(dtype), stride, shift=1 if (variant == "conv2_shifted" and i == 1) else 0), 0)
    f = y[:, :, 0]
    bias = w["lstm_b_ih"].astype(dtype) + (0 if variant == "no_b_hh" else w["lstm_b_hh"].astype(dtype))
    gx = f @ w["lstm_w_ih"].astype(dtype).T + bias
    if not want_bound:
        return gx, None
    dspec = (256 + 2) * U * (np.abs(seg) @ np.abs(basis).T)
    dmag = (np.sqrt(dspec[..., :129] ** 2 + dspec[..., 129:] ** 2)).transpose(0, 2, 1) + (1 + 2 * SQRT_ULPS) * U * mag
    layers = _fe_dense(w)
    _, first, inverse = np.unique(np.asarray(frames, np.float32), axis=0, return_index=True, return_inverse=True)
    rows = np.stack([_fe_bound_one(layers, mag[n], dmag[n]) for n in first])   # equal frames share a bound
    return gx, rows[np.asarray(inverse).ravel()]


FE_SHAPES = (((1, 2049, 512), (0, 0, 1)), ((63, 2048, 513), (1, 0, 1)), ((511, 2047, 2049), (4, 1, 0)), ((512, 1, 2048), (0, 4, 1)))
FE_INPUTS = ("speech", "fullscale", "nyquist", "dc")
FE_CASES = [(s, inp) for s in range(len(FE_SHAPES)) for inp in FE_INPUTS]


@functools.lru_cache(maxsize=None)
def fe_case(shape, inp):
    """three items in one launch: counts, extras, the packed samples"""
    counts, extras = FE_SHAPES[shape]
    total = sum(counts)
    if inp == "speech":
        from whisperlive_amd.synthetic import speech_like_pcm
        pcm = speech_like_pcm(1.0, seed=40 + shape)[3000:3000 + total].copy()
    elif inp == "fullscale":
        pcm = np.random.default_rng([shape, 1]).choice(np.asarray([-1.0, 1.0], np.float32), total)
    elif inp == "nyquist":
        pcm = np.where(np.arange(total) % 2 == 0, 1.0, -1.0).astype(np.float32)      # only bin 128 is large
    else:
        pcm = np.concatenate([np.full(n, v, np.float32) for n, v in zip(counts, (0.5, -1.0, 0.25))])
    pcm = np.ascontiguousarray(pcm, np.float32)
    pcm.setflags(write=False)
    return dict(shape=shape, inp=inp, counts=counts, extras=extras, pcm=pcm, T=[windows_of(n, e) for n, e in zip(counts, extras)])


def fe_items(c):
    off = np.concatenate([[0], np.cumsum(c["counts"])])
    return [c["pcm"][off[i]:off[i + 1]] for i in range(len(c["counts"]))]


def fe_ref(c, dtype=np.float64, variant=None, family="base"):
    """gx [sum T][512] of the launch and its bound"""
    frames, start = [], 0
    for x, e in zip(fe_items(c), c["extras"]):
        before = np.zeros(64, np.float32)
        k = min(64, start)
        if k:
            before[64 - k:] = c["pcm"][start - k:start]
        frames.append(fe_frames(x, e, before, variant))
        start += x.shape[0]
    return fe_rows(weights(family), np.concatenate(frames), dtype, variant)


def fe_silent_rows(c):
    """the packed rows whose whole 576-sample frame is zero (extra windows behind a zero tail): each must equal the row of silence"""
    fr = np.concatenate([fe_frames(x, e) for x, e in zip(fe_items(c), c["extras"])])
    return np.flatnonzero(~fr.any(axis=1))


@functools.lru_cache(maxsize=None)
def fe_silence_row(family="base"):
    return fe_rows(weights(family), np.zeros((1, 576), np.float32))


# ------------------------------------------------------------------ recurrence
LSTM_WRONGS = ("gate_order_iofg", "whh_quarters", "no_reset")
LSTM_PATTERNS = ("gauss", "sat30", "sat100", "climb", "small_c")
LSTM_TS = {"one": (65,), "ragged": (3, 65, 1), "table": tuple(1 + k % 3 for k in range(64))}
LSTM_FAMILIES = ("base", "scaled")
LSTM_CASES = ([(f, p, ts) for f in LSTM_FAMILIES for p in LSTM_PATTERNS for ts in ("ragged", "table")] +
              [(f, "gauss", "one") for f in LSTM_FAMILIES])


def lstm_gx(pattern, T, item):
    """the injected gate rows [T][512] (i, f, g, o) of one item"""
    rng = np.random.default_rng([LSTM_PATTERNS.index(pattern), T, item, 7])
    if pattern == "gauss":
        g = rng.standard_normal((T, 512))
    elif pattern in ("sat30", "sat100"):                # every gate of every unit fully closed or open, at random per step
        g = rng.choice([-1.0, 1.0], (T, 512)) * (30.0 if pattern == "sat30" else 100.0)
    elif pattern == "climb":                            # i = f = g = +30: c grows by 1 per step, past 44.4 where E(2c) = inf; h follows o
        g = np.full((T, 512), 30.0)
        g[:, 384:] = rng.standard_normal((T, 128))
    else:                                               # c' = sigmoid(-6.9) tanh(30) + sigmoid(-30) c: held near 1e-3, tanh cancels
        g = np.empty((T, 512))
        g[:, :128] = math.log(1e-3 / (1 - 1e-3)) + 0.05 * rng.standard_normal((T, 128))
        g[:, 128:256] = -30.0
        g[:, 256:384] = 30.0
        g[:, 384:] = 1.5 * rng.standard_normal((T, 128))
    return g.astype(np.float32)


def _lstm_mats(w, dtype, variant):
    whh = w["lstm_w_hh"].astype(dtype)
    if variant == "whh_quarters":                       # lane q given the columns of quarter q + 1
        whh = np.concatenate([whh[:, 32 * ((q + 1) % 4): 32 * ((q + 1) % 4) + 32] for q in range(4)], axis=1)
    order = (0, 2, 3, 1) if variant == "gate_order_iofg" else (0, 1, 2, 3)     # where i, f, g, o are taken from when the rows are i, o, f, g
    return whh, order


def lstm_ref(w, gx, dtype=np.float64, variant=None, state=None, want_bound=True):
    """one item: gx [T][512] -> h [T][128], its bound [T][128] (None unless asked for in float64), the final (h, c)"""
    whh, order = _lstm_mats(w, dtype, variant)
    gx = np.asarray(gx, dtype)
    T = gx.shape[0]
    want_bound = want_bound and dtype == np.float64 and variant is None and state is None
    h = np.zeros(H, dtype) if state is None else np.asarray(state[0], dtype)
    c = np.zeros(H, dtype) if state is None else np.asarray(state[1], dtype)
    hs = np.empty((T, H), dtype)
    bound = np.empty((T, H)) if want_bound else None
    blk = lambda v, k: v[order[k] * H: order[k] * H + H]
    if want_bound:
        awhh = np.abs(whh)
        Wi, Wf, Wg, Wo = (whh[k * H:(k + 1) * H] for k in range(4))
        Qh = np.zeros((H, T, 2 * H))                    # rows of h_t against the sources (r_c, r_h) of every step s <= t
        Qc = np.zeros((H, T, 2 * H))
        rho = np.zeros((T, 2 * H))
        eye = np.eye(H)
    with np.errstate(over="ignore"):
        for t in range(T):
            pre = gx[t] + whh @ h
            xi, xf, xg, xo = (blk(pre, k) for k in range(4))
            i, f, o = (dtype(1) / (dtype(1) + np.exp(-x)) for x in (xi, xf, xo))
            g = np.tanh(xg)
            c_prev = c
            c = f * c_prev + i * g
            th = np.tanh(c)
            hn = o * th
            if want_bound:
                rpre = LSTM_DOT_U * U * (np.abs(gx[t]) + awhh @ np.abs(h))
                ri, rf, rg, ro = (rpre[k * H:(k + 1) * H] for k in range(4))
                di, df, do = (_sig(x) * _sig(-x) for x in (xi, xf, xo))          # s (1 - s)
                dg = 4 * _sig(2 * xg) * _sig(-2 * xg)                            # 1 - tanh^2
                es = lambda x, s, d: d * eps_exp(x) + s * (1 + 2 * RCP_ULPS) * U + FLOOR
                ei, ef, eo = di * ri + es(xi, i, di), df * rf + es(xf, f, df), do * ro + es(xo, o, do)
                eg = dg * rg + 2 * es(2 * xg, _sig(2 * xg), dg / 4) + U * np.abs(g)
                rho_c = np.abs(c_prev) * ef + np.abs(g) * ei + i * eg + 2 * U * (np.abs(f * c_prev) + np.abs(i * g))
                r = _sig(-2 * c)                                                 # 1 / (1 + exp(2c))
                eth = 2 * r * (_sig(2 * c) * eps_exp(2 * c) + (1 + 2 * RCP_ULPS) * U) + U * np.abs(th) + 2 * FLOOR
                rho_h = np.abs(th) * eo + o * eth + U * np.abs(hn)
                dth = 4 * _sig(2 * c) * _sig(-2 * c)
                dhc = o * dth                                                     # dh' / dc'
                B = (c_prev * df)[:, None] * Wf + (g * di)[:, None] * Wi + (i * dg)[:, None] * Wg        # dc' / dh
                if t:
                    qh = Qh[:, :t].reshape(H, -1)
                    nqc = (B @ qh).reshape(H, t, 2 * H) + f[:, None, None] * Qc[:, :t]
                    nqh = dhc[:, None, None] * nqc + (((th * do)[:, None] * Wo) @ qh).reshape(H, t, 2 * H)
                    for q in (nqc, nqh):                 # (products of saturated derivatives reach the denormals, which only cost
                        q[np.abs(q) < 1e-150] = 0        # time: what is dropped is far below FLOOR)
                    Qc[:, :t], Qh[:, :t] = nqc, nqh
                Qc[:, t, :H] = eye
                Qh[:, t, :H] = np.diag(dhc)
                Qh[:, t, H:] = eye
                rho[t, :H], rho[t, H:] = rho_c, rho_h
                bound[t] = SLACK * np.einsum("jsk,sk->j", np.abs(Qh[:, :t + 1]), rho[:t + 1]) + FLOOR
            h = hn
            hs[t] = h
    return hs, bound, (h, c)


@functools.lru_cache(maxsize=None)
def lstm_item_ref(family, pattern, T, item):
    """(gx, h, bound) of one item, computed once and shared (read-only)"""
    gx = lstm_gx(pattern, T, item)
    hs, b, _ = lstm_ref(weights(family), gx)
    for a in (gx, hs, b):
        a.setflags(write=False)
    return gx, hs, b


def lstm_case(family, pattern, ts):
    Ts = LSTM_TS[ts]
    return dict(family=family, pattern=pattern, Ts=Ts, items=[lstm_item_ref(family, pattern, T, k) for k, T in enumerate(Ts)])


def lstm_wrong(family, pattern, ts, variant, dtype=np.float64):
    """the packed h rows [sum T][128] of a launch under a wrong variant ("no_reset": an item starts from its predecessor's final state;
    None with dtype float32: the float32 run of the restatement)"""
    out, state = [], None
    for k, T in enumerate(LSTM_TS[ts]):
        gx = lstm_gx(pattern, T, k)
        hs, _, state = lstm_ref(weights(family), gx, dtype, None if variant == "no_reset" else variant,
                                state if variant == "no_reset" else None, want_bound=False)
        out.append(hs)
    return np.concatenate(out)


def hs_layout(h, copies="same"):
    """[T][128] -> [T][512] float32, [unit][4 copies]; copies = "differ": copies 1..3 hold something else (k - h)"""
    h = np.asarray(h, np.float32)
    out = np.repeat(h[:, :, None], 4, axis=2)
    if copies == "differ":
        for k in (1, 2, 3):
            out[:, :, k] = np.float32(k) - h
    return np.ascontiguousarray(out.reshape(h.shape[0], 512))


# ------------------------------------------------------------------ output layer
OUT_WRONGS = ("no_relu", "copy1")
OUT_TARGETS = (0.0, 20.0, -20.0, 100.0, -100.0, None)      # the pre-activation of a row; None: Gaussian h
OUT_CASES = [(1, r) for r in range(6)] + [(T, r) for T in (3, 4, 5) for r in (0, 3)]


@functools.lru_cache(maxsize=None)
def out_case(T, rot, family="base"):
    """hs [T][512] whose rows reach the pre-activations OUT_TARGETS[rot ...] through the units whose weight has the sign of the target;
    every other unit is negative (the ReLU takes it out); copies 1..3 differ from copy 0"""
    w = weights(family)
    ow, ob = w["out_w"].astype(np.float64), float(w["out_b"][0])
    rng = np.random.default_rng([T, rot, 9])
    h = np.empty((T, H))
    for t in range(T):
        x = OUT_TARGETS[(rot + t) % 6]
        if x is None:
            h[t] = rng.standard_normal(H)
            continue
        h[t] = -rng.uniform(0.1, 2.0, H)
        v = x - ob
        use = ow * v > 0
        if use.any():
            h[t, use] = v * ow[use] / (ow[use] ** 2).sum()
    hs = hs_layout(h, "differ")
    hs.setflags(write=False)
    return dict(T=T, rot=rot, hs=hs)


def out_ref(c, dtype=np.float64, variant=None, family="base"):
    """probs [T] and its bound: sigmoid(out_w . relu(copy 0) + out_b)"""
    w = weights(family)
    ow, ob = w["out_w"].astype(dtype), dtype(w["out_b"][0])
    h = c["hs"].reshape(c["T"], H, 4)[:, :, 1 if variant == "copy1" else 0].astype(dtype)
    a = h if variant == "no_relu" else np.maximum(h, 0)
    x = a @ ow + ob
    with np.errstate(over="ignore"):
        p = dtype(1) / (dtype(1) + np.exp(-x))
    if dtype != np.float64 or variant is not None:
        return p, None
    dx = OUT_DOT_U * U * (np.abs(a) @ np.abs(ow) + abs(ob))
    d = _sig(x) * _sig(-x)
    b = d * (dx + eps_exp(x)) + p * (1 + 2 * DIV_ULPS) * U
    return p, SLACK * b + FLOOR


# ------------------------------------------------------------------ the hooks
def _p(a, ct, name=None, null=()):
    import ctypes as C
    return None if (name in null or a is None) else a.ctypes.data_as(C.POINTER(ct))


def filled(n):
    a = np.full(n, FILL, np.float32)
    a[1::2] = -FILL
    return a


def make_model(family="base"):
    from whisperlive_amd import vad
    return vad.SileroHIPModel(weights(family), device=0)


def run_frontend(m, pcm, counts, extras, cap, null=(), n=None):
    """-> rc, gx [cap * 512 + GUARD], its initial words; `null` names pointers passed as null"""
    import ctypes as C
    counts = np.ascontiguousarray(counts, np.int64)
    ex = None if extras is None else np.ascontiguousarray(extras, np.int32)
    pcm = np.ascontiguousarray(pcm, np.float32)
    out = filled(max(cap, 1) * 512 + GUARD)
    init = out.copy()
    rc = m.lib.wlx_vad_debug_frontend(None if "v" in null else m.handle, _p(pcm, C.c_float, "pcm", null), _p(counts, C.c_int64, "counts", null),
                                      _p(ex, C.c_int32, "extras", null), len(counts) if n is None else n, _p(out, C.c_float, "gx", null), cap)
    return rc, out, init


def run_lstm(m, gx, Ts, cap, null=(), n=None):
    import ctypes as C
    Ts = np.ascontiguousarray(Ts, np.int32)
    gx = np.ascontiguousarray(gx, np.float32)
    out = filled(max(cap, 1) * 512 + GUARD)
    init = out.copy()
    rc = m.lib.wlx_vad_debug_lstm(None if "v" in null else m.handle, _p(gx, C.c_float, "gx", null), _p(Ts, C.c_int32, "T", null),
                                  len(Ts) if n is None else n, _p(out, C.c_float, "hs", null), cap)
    return rc, out, init


def run_out(m, hs, T, cap, null=()):
    import ctypes as C
    hs = np.ascontiguousarray(hs, np.float32)
    out = filled(max(cap, 1) + GUARD)
    init = out.copy()
    rc = m.lib.wlx_vad_debug_out(None if "v" in null else m.handle, _p(hs, C.c_float, "hs", null), T, _p(out, C.c_float, "probs", null), cap)
    return rc, out, init
