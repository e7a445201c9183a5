"""Float64 numpy restatement of the band-merge rule of csrc/band_merge.hip (include/sos_hip.h states it).  Test infrastructure
like the oracle: the reference, not the code under test.

Per channel of a recording at sr_native > sr_low: x = the native plane (n frames), a = x at sr_low (m samples), b = the
networks' output for a (m' <= m samples), ua / ub = a and b resampled back to sr_native and cut or zero-filled to n.
    gains(a, b, hop, smooth)                  s[j], one value per hop frame of a
    interp(s, n, sr_low, sr_native, hop)      g[t], the gain of every native frame
    merge(x, ua, ub, g)                       out[t] = g[t] * (x[t] - ua[t]) + ub[t]"""
import numpy as np


def gains(a, b, hop, smooth):
    """Frame j covers samples [j hop, (j + 1) hop) cut at m = len(a); E_a = sum a^2, E_b = sum b^2 in float64, b reading zero
    from len(b) on; r = 1 where E_a == 0, else min(1, sqrt(E_b / E_a)); s[j] = mean of r[max(0, j - smooth) .. min(J - 1, j +
    smooth)] in float64, returned as float32."""
    a = np.asarray(a, dtype=np.float64)
    m = len(a)
    bz = np.zeros(m)
    bz[:len(b)] = np.asarray(b, dtype=np.float64)
    J = -(-m // hop)
    r = np.ones(J)
    for j in range(J):
        ea = float(np.sum(a[j * hop:(j + 1) * hop] ** 2))
        eb = float(np.sum(bz[j * hop:(j + 1) * hop] ** 2))
        if ea != 0.0:
            r[j] = min(1.0, np.sqrt(eb / ea))
    s = np.asarray([np.mean(r[max(0, j - smooth):min(J - 1, j + smooth) + 1]) for j in range(J)])
    return s.astype(np.float32)


def interp(s, n, sr_low, sr_native, hop):
    """g[t], 0 <= t < n: linear interpolation of s at the frame-centre position p = (t + 0.5) / (rho hop) - 0.5 with rho =
    sr_native / sr_low, s[0] for p <= 0 and s[J - 1] for p >= J - 1; float64 (the kernel rounds it to float32)."""
    s = np.asarray(s, dtype=np.float64)
    J = len(s)
    rho = float(sr_native) / sr_low
    p = (np.arange(n, dtype=np.float64) + 0.5) / (rho * hop) - 0.5
    g = np.empty(n)
    below, above = p <= 0.0, p >= J - 1
    g[below], g[above] = s[0], s[J - 1]
    mid = ~(below | above)
    i = np.floor(p[mid]).astype(np.int64)
    g[mid] = s[i] + (p[mid] - i) * (s[i + 1] - s[i])
    return g


def merge(x, ua, ub, g):
    """out[t] = g[t] * (x[t] - ua[t]) + ub[t] in float64; g: an array, or a scalar (1.0 = 'keep')."""
    x, ua, ub = (np.asarray(v, dtype=np.float64) for v in (x, ua, ub))
    return np.asarray(g, dtype=np.float64) * (x - ua) + ub
