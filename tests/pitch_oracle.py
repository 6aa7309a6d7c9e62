"""Numpy statement of the pitch extraction ev_pitch computes (include/evhip.h, steps 1-7): the float64 yardstick, and the same steps in the
kernel's arithmetic class (float32 terms, float32 sequential sums) as the measure of what float32 costs (tests/test_pitch.py,
tests/test_gpu_pitch.py).  Signals of known F0 come from ``harmonic``."""
import numpy as np

from emotivoice_amd.pitch import PitchConfig


def to_float(wav):
    wav = np.asarray(wav).reshape(-1)
    if wav.dtype == np.int16:
        return wav.astype(np.float32) / np.float32(32768.0)
    return wav.astype(np.float32)


def harmonic(f0_track, amps, sr=16000):
    """sum_h amps[h - 1] sin(h phi), phi = 2 pi cumsum(f0) / sr: a signal whose F0 at sample n is f0_track[n].  float64."""
    phi = 2.0 * np.pi * np.cumsum(np.asarray(f0_track, np.float64)) / sr
    return sum(a * np.sin((h + 1) * phi) for h, a in enumerate(amps))


def fill(f0):
    """Step 6: the continuous track of an (T,) F0 array (0 = unvoiced), float64 arithmetic rounded once to f0's dtype."""
    f0 = np.asarray(f0)
    out = np.zeros(f0.shape, np.float64)
    v = np.nonzero(f0 > 0)[0]
    if v.size == 0:
        return out.astype(f0.dtype)
    f = f0.astype(np.float64)
    t = np.arange(f0.size)
    nxt = np.searchsorted(v, t, side="left")            # index into v of the next voiced frame >= t
    prv = np.searchsorted(v, t, side="right") - 1       # ... of the previous voiced frame <= t
    for i in range(f0.size):
        if prv[i] < 0:
            out[i] = f[v[0]]
        elif nxt[i] >= v.size:
            out[i] = f[v[-1]]
        elif v[prv[i]] == v[nxt[i]]:
            out[i] = f[i]
        else:
            a, b = int(v[prv[i]]), int(v[nxt[i]])
            out[i] = f[a] + ((f[b] - f[a]) / (b - a)) * (i - a)
    return out.astype(f0.dtype)


def standardise(cont, mean, std):
    """Step 7 as the device evaluates it: float32 subtraction and division."""
    return (np.asarray(cont, np.float32) - np.float32(mean)) / np.float32(std)


def frames_of(x, cfg):
    """(T, S) frames of step 1: frame t = the S = W + tau_max + 1 samples from t hop - S // 2, zeros outside the utterance."""
    tau_max = cfg.tau_range()[1]
    S = cfg.win + tau_max + 1
    T = x.size // cfg.hop + 1
    pad = np.zeros(S // 2 + (T - 1) * cfg.hop + S, x.dtype)
    n = min(x.size, pad.size - S // 2)
    pad[S // 2:S // 2 + n] = x[:n]
    return np.lib.stride_tricks.sliding_window_view(pad, S)[::cfg.hop][:T]


def pitch64(wav, cfg=None, dtype=np.float64, sequential=False, stats=(0.0, 1.0)):
    """Steps 1-7 for one utterance (float or int16).  dict(f0, aperiodicity, cont, pitch, tau (-1 = unvoiced), margin, voiced).
    dtype / sequential: np.float32 and True evaluate steps 2-5 in the kernel's arithmetic class -- float32 differences and squares, float32
    sums in np.cumsum's sequential order, the running sum of step 3 in float64 on those float32 d, d' rounded to float32.
    margin[t]: how far the frame's decisions are from flipping -- the smallest of |d'[tau] - threshold| over the lags examined,
    |d'[k + 1] - d'[k]| over the walk and at its end, and |E0 / (W silence_rms^2) - 1|."""
    cfg = cfg or PitchConfig()
    x = to_float(wav).astype(dtype)
    tau_min, tau_max = cfg.tau_range()
    W, sr = cfg.win, cfg.sample_rate
    thr = float(np.float32(cfg.threshold))
    e_floor = float(W) * float(np.float32(cfg.silence_rms)) ** 2
    fr = frames_of(x, cfg)
    T = fr.shape[0]
    NL = tau_max + 2
    f0 = np.zeros(T, np.float64)
    ap = np.ones(T, np.float64)
    tau_out = np.full(T, -1, np.int64)
    margin = np.full(T, np.inf)
    for t in range(T):
        s = fr[t]
        a = s[:W]
        sq = a * a
        E0 = float(np.cumsum(sq)[-1]) if sequential else float(sq.sum(dtype=np.float64))
        u = a[None, :] - np.lib.stride_tricks.sliding_window_view(s, W)[:NL]
        u = u * u
        d = np.cumsum(u, axis=1)[:, -1] if sequential else u.sum(axis=1, dtype=dtype)
        cs = np.zeros(NL, np.float64)
        cs[1:] = np.cumsum(d[1:].astype(np.float64))
        dp = np.ones(NL, np.float64)
        k = np.arange(NL)
        ok = cs > 0
        ok[0] = False
        dp[ok] = d[ok].astype(np.float64) * k[ok] / cs[ok]
        dp = dp.astype(dtype)
        m = abs(E0 / e_floor - 1.0) if e_floor > 0 else np.inf
        if E0 < e_floor:
            margin[t] = m
            continue
        tau = -1
        for k in range(tau_min, tau_max + 1):
            m = min(m, abs(float(dp[k]) - thr))
            if dp[k] < thr:
                tau = k
                break
        if tau >= 0:
            while tau + 1 <= tau_max:
                m = min(m, abs(float(dp[tau + 1]) - float(dp[tau])))
                if not dp[tau + 1] < dp[tau]:
                    break
                tau += 1
            y0, y1, y2 = float(dp[tau - 1]), float(dp[tau]), float(dp[tau + 1])
            den = y0 - 2.0 * y1 + y2
            off = 0.5 * (y0 - y2) / den if den > 0 else 0.0
            off = min(0.5, max(-0.5, off))
            f0[t] = sr / (tau + off)
            ap[t] = y1
            tau_out[t] = tau
        margin[t] = m
    out_t = np.float32 if dtype == np.float32 else np.float64
    f0 = f0.astype(out_t)
    cont = fill(f0)
    if out_t == np.float32:
        pitch = standardise(cont, stats[0], stats[1])
    else:
        pitch = (cont - float(np.float32(stats[0]))) / float(np.float32(stats[1]))
    return dict(f0=f0, aperiodicity=ap.astype(out_t), cont=cont, pitch=pitch, tau=tau_out, margin=margin, voiced=tau_out >= 0)


def rel_error(f0, f064):
    """max over the frames voiced in the yardstick of |f0 - f064| / f064."""
    f0, f064 = np.asarray(f0, np.float64), np.asarray(f064, np.float64)
    v = f064 > 0
    return float((np.abs(f0 - f064)[v] / f064[v]).max()) if v.any() else 0.0


def abs_error(x, x64):
    return float(np.abs(np.asarray(x, np.float64) - np.asarray(x64, np.float64)).max()) if np.asarray(x).size else 0.0
