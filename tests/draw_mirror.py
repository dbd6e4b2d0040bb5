"""A numpy restatement of the contract of cavmd_draw_fill (include/cavmd.h, "the step inputs of a batch, drawn on the device"):
the Philox4x32-10 rounds on uint64 arithmetic, the exact step from words to doubles, Box-Muller, the Marsaglia-Tsang gamma
sampler with its try order, and the dt rule.  Everything is vectorised over items.

What is exact and what is not.  The generator, the words-to-doubles step, +, -, *, / and sqrt are the same IEEE operations
here and on the device: those results are compared bit for bit.  log, exp and cospi are library functions on either side.
The HIP math API documents at most 2 ulp for the three in double precision and glibc / numpy less than 1 ulp for theirs; each
side is taken to be within FUNCTION_ULP = 4 ulp of the true value, so two results differ by at most

    DELTA = 2 * FUNCTION_ULP * EPS            (relative to the function value)

and that is propagated through each expression below, with EPS for every rounding that follows (first order; the products
of two such terms are 1e-32 and dropped, and covered by rounding every count of EPS up).  cospi is taken here from sin / cos
of pi * r after an EXACT reduction of the argument to |r| <= 1/4 (the argument is a multiple of 2^-52, so the subtractions
are exact), which keeps it relatively accurate next to its zeros; pi * r adds 1.5 ulp to the argument, inside FUNCTION_ULP.

    normal      n = sqrt(-2 log u1) cospi(2 u2):  log DELTA -> sqrt DELTA / 2 + EPS; cospi DELTA; the product EPS:
                |dn| <= NORMAL_REL |n|,  NORMAL_REL = 1.5 DELTA + 4 EPS = 16 EPS
    gamma       v1 = 1 + c x with x a normal:  |dv1| <= |c x| (NORMAL_REL + EPS) + EPS |v1|;  rho = |dv1| / |v1|;
                v = v1^3: 3 rho + 2 EPS;  the variate d v: |dg| <= (3 rho + 4 EPS) |g|
                the margin m = ((x^2 / 2 + d) - d v) + d log v - log u of the acceptance test moves by at most
                  DELTA |log u| + (x^2 / 2)(2 NORMAL_REL + 2 EPS) + d |v| (3 rho + 3 EPS) + d (3 rho + 2 EPS + DELTA |log v|)
                  + 4 EPS (x^2 / 2 + d + d |v| + d |log v|)
                a try with |m| at or below that, or |v1| at or below |dv1|, may legitimately go the other way on the device:
                the draw is `ambiguous`
    shape < 1   times exp(y), y = log(u) / a: |dy| <= |y| (DELTA + EPS); exp: |dy| + DELTA; the product EPS
    c           exp(-dt / tau) with dt exact: DELTA (C_REL)
    tolerance   target - D E, D = target - initial, E = exp(-elapsed / tc) with elapsed exact:
                |dtol| <= |D| E (DELTA + 2 EPS) + EPS |tol|
None of this is fitted to what a GPU returned."""
import math

import numpy as np

EPS = 2.0 ** -52
FUNCTION_ULP = 4.0
DELTA = 2.0 * FUNCTION_ULP * EPS
NORMAL_REL = 1.5 * DELTA + 4.0 * EPS
C_REL = DELTA
GAMMA_TRIES = 16

PURPOSE_LANGEVIN_XY, PURPOSE_LANGEVIN_Z, PURPOSE_NORMAL, PURPOSE_BOOST, PURPOSE_GAMMA_TRY = 0, 1, 2, 3, 16
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_U32 = np.uint64(32)
KEY_STRIDE = 0x9E3779B97F4A7C15


def item_key(seed: int, i: int) -> int:
    """the key LangevinBathBatch and BatchThermalizer give system i (_capi.bath_item_key)"""
    return (int(seed) + KEY_STRIDE * (int(i) + 1)) % 2 ** 64


def philox(counter, key):
    """Philox4x32-10: counter (..., 4) and key (..., 2) of 32-bit values held in uint64 -> (..., 4) uint64 words."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & _MASK for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> _U32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _U32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def block(seed, draws, item, purpose):
    """The four words of counter (draws low, draws high, item, purpose) under the key (seed low, seed high)."""
    draws, item, purpose = np.broadcast_arrays(np.asarray(draws, dtype=np.uint64), np.asarray(item, dtype=np.uint64),
                                               np.asarray(purpose, dtype=np.uint64))
    counter = np.stack([draws & _MASK, draws >> _U32, item, purpose], axis=-1)
    seed = np.uint64(seed)
    return philox(counter, np.array([seed & _MASK, seed >> _U32], dtype=np.uint64))


def bits53(w_hi, w_lo):
    return (w_hi << np.uint64(21)) | (w_lo >> np.uint64(11))


def unit(w_hi, w_lo):
    """[0, 1), exact"""
    return bits53(w_hi, w_lo).astype(np.float64) * 2.0 ** -53


def log_arg(w_hi, w_lo):
    """(0, 1], exact"""
    return (bits53(w_hi, w_lo) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def cospi(t):
    """cos(pi t) for t in [0, 2] a multiple of 2^-52: the argument is reduced exactly to |r| <= 1/4."""
    t = np.asarray(t, dtype=np.float64)
    q = np.floor(2.0 * t + 0.5)                 # the nearest multiple of 1/2
    r = t - 0.5 * q                             # exact
    q = q.astype(np.int64) & 3
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def normal(seed, draws, item, purpose):
    w = block(seed, draws, item, purpose)
    return np.sqrt(-2.0 * np.log(log_arg(w[..., 0], w[..., 1]))) * cospi(2.0 * unit(w[..., 2], w[..., 3]))


def langevin_uniforms(seed, draws, item):
    """(..., 3) variates in [-1, 1), exact"""
    xy = block(seed, draws, item, PURPOSE_LANGEVIN_XY)
    z = block(seed, draws, item, PURPOSE_LANGEVIN_Z)
    return np.stack([2.0 * unit(xy[..., 0], xy[..., 1]) - 1.0, 2.0 * unit(xy[..., 2], xy[..., 3]) - 1.0,
                     2.0 * unit(z[..., 0], z[..., 1]) - 1.0], axis=-1)


def gamma_ge1(seed, draws, item, a):
    """Marsaglia-Tsang for shapes a >= 1 -> dict of arrays: value, bound (on |device - value|), tries (1-based number of the
    accepted try; GAMMA_TRIES + 1 if none was), exhausted (bool), ambiguous (bool: some try up to the accepted one could
    legitimately go the other way on the device)."""
    draws, item, a = np.broadcast_arrays(np.asarray(draws, dtype=np.uint64), np.asarray(item, dtype=np.uint64),
                                         np.asarray(a, dtype=np.float64))
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    value, bound = d.copy(), np.zeros_like(d)
    tries = np.full(d.shape, GAMMA_TRIES + 1, dtype=np.int64)
    ambiguous = np.zeros(d.shape, dtype=bool)
    pending = np.ones(d.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(GAMMA_TRIES):
            if not pending.any():
                break
            x = normal(seed, draws, item, PURPOSE_GAMMA_TRY + 2 * t)
            w = block(seed, draws, item, PURPOSE_GAMMA_TRY + 2 * t + 1)
            logu = np.log(log_arg(w[..., 0], w[..., 1]))
            v1 = 1.0 + c * x
            v = (v1 * v1) * v1
            logv = np.log(np.where(v > 0.0, v, 1.0))
            margin = ((((0.5 * x) * x + d) - d * v) + d * logv) - logu
            dv1 = np.abs(c * x) * (NORMAL_REL + EPS) + EPS * np.abs(v1)
            rho = dv1 / np.abs(v1)
            half = 0.5 * x * x
            dm = (DELTA * np.abs(logu) + half * (2.0 * NORMAL_REL + 2.0 * EPS) + d * np.abs(v) * (3.0 * rho + 3.0 * EPS)
                  + d * (3.0 * rho + 2.0 * EPS + DELTA * np.abs(logv)) + 4.0 * EPS * (half + d + d * np.abs(v) + d * np.abs(logv)))
            unsure = (np.abs(v1) <= dv1) | ((v > 0.0) & (np.abs(margin) <= dm))
            accept = (v > 0.0) & (margin > 0.0)
            ambiguous |= pending & unsure
            now = pending & accept
            value = np.where(now, d * v, value)
            bound = np.where(now, (3.0 * rho + 4.0 * EPS) * np.abs(d * v), bound)
            tries = np.where(now, t + 1, tries)
            pending &= ~accept
    return dict(value=value, bound=bound, tries=tries, exhausted=pending, ambiguous=ambiguous)


def gamma(seed, draws, item, a):
    """Gamma variates of shapes a > 0 (scale 1): a >= 1 as gamma_ge1, a < 1 as the shape-(a + 1) variate times
    exp(log(u) / a) with u the boost uniform."""
    draws, item, a = np.broadcast_arrays(np.asarray(draws, dtype=np.uint64), np.asarray(item, dtype=np.uint64),
                                         np.asarray(a, dtype=np.float64))
    small = a < 1.0
    out = gamma_ge1(seed, draws, item, np.where(small, a + 1.0, a))
    if small.any():
        w = block(seed, draws, item, PURPOSE_BOOST)
        y = np.log(log_arg(w[..., 0], w[..., 1])) / np.where(small, a, 1.0)
        boost = np.exp(y)
        rel = np.abs(y) * (DELTA + EPS) + DELTA + EPS
        value = out["value"] * boost
        out["bound"] = np.where(small, out["bound"] * boost + np.abs(value) * (rel + EPS), out["bound"])
        out["value"] = np.where(small, value, out["value"])
    return out


def fixed_columns(gamma_, kT, dt, tau):
    """(langevin_coeff, c) as cavmd_verlet_input_make and cavmd_bussi_batch_input_make take them on the host: sqrt and / are
    correctly rounded everywhere; exp is the C library's, which math.exp calls."""
    gamma_, kT, dt, tau = (np.asarray(x, dtype=np.float64) for x in np.broadcast_arrays(gamma_, kT, dt, tau))
    with np.errstate(divide="ignore", invalid="ignore"):
        coeff = np.where((gamma_ != 0.0) & (dt != 0.0), np.sqrt(6.0 * gamma_ * kT / np.where(dt != 0.0, dt, 1.0)), 0.0)
    c = np.array([math.exp(-d / t) if t != 0.0 else 0.0 for d, t in zip(dt.ravel(), tau.ravel())]).reshape(dt.shape)
    return coeff, c


ITEM_FIELDS = ("gamma", "kT", "set_T", "tau", "dof", "dt_initial", "tol_target", "tol_initial", "tol_time_constant", "dt_min",
               "dt_max")


def new_state(n):
    return dict(draws=np.zeros(n, dtype=np.uint64), dt=np.zeros(n), elapsed=np.zeros(n), tolerance=np.zeros(n),
                exhausted=np.zeros(n, dtype=np.uint64))


def time_step(it, st, adaptive, recorded, S, tolerance=None):
    """Item 5 of the contract for every item -> dict dt, coeff, c, tolerance, tolerance_bound, c_bound.  it: ITEM_FIELDS ->
    (B,) arrays; adaptive: (B,) bool; recorded: (B,) rows the item's recorder holds; S: (B,) force_mass_sum of the last one.
    tolerance: None, or (B,) tolerances to use instead of this function's own where a ramp is on (the device's, so that what
    follows from them is compared bit for bit); tolerance_bound still belongs to this function's own value."""
    B = len(adaptive)
    coeff0, c0 = fixed_columns(it["gamma"], it["kT"], it["dt_initial"], it["tau"])
    ramp = adaptive & (it["tol_time_constant"] != 0.0)
    D = it["tol_target"] - it["tol_initial"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        E = np.where(ramp, np.exp(-st["elapsed"] / np.where(ramp, it["tol_time_constant"], 1.0)), 0.0)
        own = np.where(ramp, it["tol_target"] - D * E, it["tol_target"])
        tol_bound = np.where(ramp, np.abs(D) * E * (DELTA + 2.0 * EPS) + EPS * np.abs(own), 0.0)
        tol = own if tolerance is None else np.where(ramp, tolerance, own)
        last = np.where(st["draws"] != 0, st["dt"], it["dt_initial"])
        usable = (S > 0.0) & np.isfinite(S)
        rule = np.minimum(np.maximum(np.sqrt(tol / np.where(usable, S, 1.0)), it["dt_min"]), it["dt_max"])
        dt = np.where(recorded == 0, it["dt_initial"], np.where(usable, rule, last))
        dt = np.where(adaptive, dt, it["dt_initial"])
        coeff = np.where((it["gamma"] != 0.0) & (dt != 0.0), np.sqrt(((6.0 * it["gamma"]) * it["kT"]) / np.where(dt != 0.0, dt, 1.0)),
                         0.0)
        c = np.where(it["tau"] != 0.0, np.exp(-dt / np.where(it["tau"] != 0.0, it["tau"], 1.0)), 0.0)
    return dict(dt=dt, coeff=np.where(adaptive, coeff, coeff0), c=np.where(adaptive, c, c0),
                c_bound=np.where(adaptive, C_REL * np.abs(c), 0.0), tolerance=np.where(adaptive, tol, 0.0),
                own_tolerance=np.where(adaptive, own, 0.0), tolerance_bound=tol_bound, B=B)


def step(seed, it, st, adaptive, recorded, S, tolerance=None):
    """One launch for every item (both rows, whatever the destinations) -> (verlet (B, 8), bussi (B, 8), new state, info).
    info: normal_bound, gamma_bound, gamma_ambiguous, gamma_tries, c_bound, tolerance_bound, own_tolerance."""
    B = len(adaptive)
    item = np.arange(B, dtype=np.uint64)
    ts = time_step(it, st, adaptive, recorded, S, tolerance)
    skip = (ts["dt"] == 0.0).astype(np.uint64).view(np.float64)
    verlet = np.zeros((B, 8))
    verlet[:, 0], verlet[:, 1], verlet[:, 2] = ts["dt"], it["gamma"], ts["coeff"]
    verlet[:, 3:6] = langevin_uniforms(seed, st["draws"], item)
    verlet[:, 6] = skip
    bussi = np.zeros((B, 8))
    has_normal, has_gamma = it["dof"] != 0.0, it["dof"] > 1.0
    n = normal(seed, st["draws"], item, PURPOSE_NORMAL)
    bussi[:, 0] = np.where(has_normal, n, 0.0)
    g = gamma(seed, st["draws"], item, np.where(has_gamma, (it["dof"] - 1.0) / 2.0, 1.0))
    bussi[:, 1] = np.where(has_gamma, g["value"], 0.0)
    bussi[:, 2], bussi[:, 3], bussi[:, 4] = ts["c"], it["set_T"], skip
    new = dict(draws=st["draws"] + np.uint64(1), dt=ts["dt"], elapsed=st["elapsed"] + ts["dt"], tolerance=ts["tolerance"],
               exhausted=st["exhausted"] + (has_gamma & g["exhausted"]).astype(np.uint64))
    info = dict(normal_bound=np.where(has_normal, NORMAL_REL * np.abs(n), 0.0), gamma_bound=np.where(has_gamma, g["bound"], 0.0),
                gamma_ambiguous=has_gamma & g["ambiguous"], gamma_tries=np.where(has_gamma, g["tries"], 0),
                c_bound=ts["c_bound"], tolerance_bound=ts["tolerance_bound"], own_tolerance=ts["own_tolerance"])
    return verlet, bussi, new, info
