"""TEST INFRASTRUCTURE ONLY -- numpy float64 / integer restatement of the rule by which audio_io.StreamBandMerger puts the band
above the networks' half rate back into a LIVE stream (csrc/stream_band.hip), on top of band_reference (the merge rule of whole
signals) and stream_resample_reference (resampy's running time register and the finality of a resampled output).

Notation.  x = the native stream, a = x at the low rate, b = the networks' output for a, U = the resampling back at rho = native /
low > 1 (an upsampling: scale = 1, R = 64 per wing), time(t) = the running f64 sum of 1 / rho, n(t) = floor(time(t)), hop and K =
`smooth` as in band_reference.gains (K = None: no gains, 'keep').  A stream has received n_x samples of x, m_a of a and m_b of
b, m_b <= m_a <= m_x = ceil(n_x low / native).

Finality.  Output t has the value it has for any longer stream once
  (1) n(t) + 1 + R <= m_b: neither right wing of U(a)[t], U(b)[t] is cut (stream_resample_reference, asked about m_b <= m_a);
  (2) with gains, F(t) < m_b // hop - K, F(t) = 0 for p <= 0 and floor(p) + 1 otherwise, p = (t + 0.5) / (rho hop) - 0.5: g[t]
      reads s[floor(p)] and s[F(t)] (s[0] alone for p <= 0); r[j] is final once (j + 1) hop <= m_b, s[j] once r[j + K] is -- that
      frame is whole, so it lies below J - 1 or is it, and the cut of the mean at the clip's end cannot reach s[j]; and F(t) <=
      J - 1 means p < J - 1, so the clamp at the end does not apply;
  (3) t < n_x.
Each holds for a prefix of t (time and p increase), T = the shortest of the three.  `stream` emits by this rule from prefixes
alone and asserts each fact where it uses it.

Retained.  Later outputs read x from T; a and b from max(n(T) - (R - 1), 0), and the frames of r still to come read them from
hop (m_b // hop); r from max(F(T) - 1 - K, 0).

Pending bounds, for a stream whose b trails what x gives by at most `max_lag`: m_x - m_b <= max_lag (so b trails a by no more).
With LAT = R without gains and max(R, (K + 2) hop) with them (what b must lead an output by), after every step
  T >= rho (m_b - LAT) - 2 or T = n_x      [T_rs ~ rho (m_b - R); T_g >= (m_b // hop - K - 0.5) rho hop - 1.5]
  x: n_x - T                 <= ceil(rho (max_lag + LAT)) + 2                 (n_x <= rho m_x)
  b: m_b - first             <= LAT + R + 2                                   (n(T) >= T / rho - 1)
  a: m_a - first             <= max_lag + LAT + R + 2
  r: m_b // hop - first_r    <= max(2 K + 1, K + ceil(R / hop) + 2)           (gain-limited: F(T) >= m_b // hop - K; else p(T) >=
                                                                               (m_b - R) / hop - 0.5)
`bounds(max_lag)` states them; `stream` asserts them after every step.

Close.  n, m = len(a) and m' = len(b) are known: the outputs [T, n) follow with band_reference's arguments -- U(a) of m samples,
U(b) of m' samples and zero from int(m' rho) on, all J = ceil(m / hop) frames of r (b reading zero from m' on), the mean cut at
J - 1 and p clamped there.  The concatenated output has exactly n samples."""
import numpy as np

import band_reference as BR
import stream_resample_reference as SR


class Rule:
    def __init__(self, low_sr, native_sr, hop, smooth=None):
        assert native_sr > low_sr
        self.low_sr, self.native_sr, self.hop, self.K = low_sr, native_sr, int(hop), smooth
        self.up = SR.Rule(low_sr, native_sr)
        self.rho, self.R = self.up.ratio, self.up.R
        assert self.up.scale == 1.0 and self.up.index_step == self.up.num_table
        self.frame = self.rho * float(self.hop)

    def pos(self, t):
        return (np.asarray(t, dtype=np.float64) + 0.5) / self.frame - 0.5

    def last(self, t):
        """F(t): the last frame of s that g[t] reads while no end clamps it."""
        p = self.pos(t)
        return np.where(p > 0.0, np.floor(p) + 1, 0).astype(np.int64)

    def n_of(self, t):
        return int(self.up.time(t + 1)[t])

    def ready(self, m_b, n_x):
        """(T, first x, first a, first b, first r) after m_b samples of b and n_x of x."""
        T = min(self.up.ready(m_b)[0], n_x)
        if self.K is not None:
            final_s = m_b // self.hop - self.K                       # s[j] is final for j below this
            if final_s < 1:
                T = 0
            elif int(self.last(T)) >= final_s:
                est = int((final_s - 0.5) * self.frame)              # p(t) = final_s - 1 near here
                cand = np.arange(max(est - 3, 0), est + 4)
                hit = cand[self.last(cand) >= final_s]
                T_g = int(hit[0])
                assert T_g == 0 or (T_g > cand[0] and int(self.last(T_g - 1)) < final_s)
                T = min(T, T_g)
        first = max(self.n_of(T) - (self.R - 1), 0)
        first_r = 0
        if self.K is not None:
            first = min(first, self.hop * (m_b // self.hop))
            first_r = max(int(self.last(T)) - 1 - self.K, 0)
        return T, T, first, first, first_r

    def bounds(self, max_lag):
        """The most x, a, b samples and r frames retained after a step of a stream with m_x - m_b <= max_lag."""
        K = self.K
        lat = self.R if K is None else max(self.R, (K + 2) * self.hop)
        return dict(x=int(np.ceil(self.rho * (max_lag + lat))) + 2, a=max_lag + lat + self.R + 2, b=lat + self.R + 2,
                    r=0 if K is None else max(2 * K + 1, K + -(-self.R // self.hop) + 2))

    def _ratio(self, a, b, j, m_a, m_b):
        """r[j] from the prefixes a[:m_a], b[:m_b] (b reads zero from m_b on), with band_reference.gains's statements."""
        hop = self.hop
        bz = np.zeros(m_a)
        bz[:m_b] = b[:m_b]
        ea = float(np.sum(a[:m_a][j * hop:(j + 1) * hop] ** 2))
        eb = float(np.sum(bz[j * hop:(j + 1) * hop] ** 2))
        return 1.0 if ea == 0.0 else min(1.0, np.sqrt(eb / ea))

    def _gain(self, r, t_lo, t_hi, J):
        """g[t_lo .. t_hi) from the frames r (a dict j -> r[j]); J None: the stream is open."""
        K = self.K
        p = self.pos(np.arange(t_lo, t_hi))
        i = np.where(p > 0.0, np.floor(p), 0).astype(np.int64)
        if J is not None:
            i = np.minimum(i, J - 1)
        s = {}
        for j in set(i.tolist()) | set((i + 1).tolist()):
            if J is not None and j > J - 1:
                continue
            if J is None and j + K not in r:
                continue                                             # asserted below where it is read
            hi = j + K if J is None else min(J - 1, j + K)
            s[j] = float(np.float32(np.mean(np.asarray([r[q] for q in range(max(0, j - K), hi + 1)]))))
        g = np.empty(len(p))
        for k, (pk, ik) in enumerate(zip(p.tolist(), i.tolist())):
            if pk <= 0.0:
                g[k] = s[0]
            elif J is not None and pk >= J - 1:
                g[k] = s[J - 1]
            else:
                g[k] = s[ik] + (pk - ik) * (s[ik + 1] - s[ik])       # KeyError: a frame that is not final was asked for
        return g

    def stream(self, x, a, b, steps, max_lag):
        """x, a, b fed in steps (c_x, c_a, c_b) that sum to their lengths, then closed -> (the emitted pieces, one per step and
        one for the close; the most x, a, b samples and r frames pending after a step).  Reads prefixes only; asserts finality
        and the pending bounds at every step."""
        x, a, b = (np.asarray(v, dtype=np.float64) for v in (x, a, b))
        n, m, mp, hop, K = len(x), len(a), len(b), self.hop, self.K
        assert [sum(c) for c in zip(*steps)] == [n, m, mp] and 1 <= mp <= m and int(m * self.rho) >= n
        bound, most = self.bounds(max_lag), dict(x=0, a=0, b=0, r=0)
        n_x = m_a = m_b = T = 0
        r, pieces = {}, []

        def emit(t_lo, t_hi, J):
            xa, xb = a[:m_a], b[:m_b]                                 # nothing past the prefixes can be read
            ua, fa = self.up.outputs(xa, m_a, t_lo, t_hi)
            v_hi = t_hi if J is None else min(max(int(m_b * self.rho), t_lo), t_hi)      # U(b) is zero from int(m' rho) on
            ub, fb = self.up.outputs(xb, m_b, t_lo, v_hi)
            ub = np.concatenate([ub, np.zeros(t_hi - v_hi)])
            if J is None:
                assert fa and fb
            g = 1.0 if K is None else self._gain(r, t_lo, t_hi, J)
            return BR.merge(x[t_lo:t_hi], ua, ub, g)

        for c_x, c_a, c_b in steps:
            n_x, m_a, m_b = n_x + int(c_x), m_a + int(c_a), m_b + int(c_b)
            m_x = -(-n_x * self.low_sr // self.native_sr)
            assert m_b <= m_a <= m_x and m_x - m_b <= max_lag, (n_x, m_a, m_b, max_lag)
            if K is not None:
                for j in range(len(r), m_b // hop):                  # whole frames of final samples
                    r[j] = self._ratio(a, b, j, m_a, m_b)
            T_new, f_x, f_a, f_b, f_r = self.ready(m_b, n_x)
            assert T <= T_new <= n_x and T_new <= int(m_b * self.rho)
            pieces.append(emit(T, T_new, None) if T_new > T else np.zeros(0))
            T = T_new
            pend = dict(x=n_x - f_x, a=m_a - f_a, b=m_b - f_b, r=(m_b // hop - f_r) if K is not None else 0)
            for k, v in pend.items():
                assert 0 <= v <= bound[k], (k, v, bound[k], n_x, m_a, m_b)
                most[k] = max(most[k], v)
        assert (n_x, m_a, m_b) == (n, m, mp)
        J = -(-m // hop)
        if K is not None:
            for j in range(m_b // hop, J):                           # the frames b does not fill: they read zero from m' on
                r[j] = self._ratio(a, b, j, m_a, m_b)
        pieces.append(emit(T, n, J) if n > T else np.zeros(0))
        return pieces, most


def whole(rule, x, a, b):
    """band_reference's result for the whole signals: what the pieces of Rule.stream concatenate to."""
    from oracle import wave_io as owio
    n = len(x)
    ua = owio.resample(np.asarray(a, dtype=np.float64), rule.low_sr, rule.native_sr, fix=False)[:n]
    ub = np.zeros(n)
    rb = owio.resample(np.asarray(b, dtype=np.float64), rule.low_sr, rule.native_sr, fix=False)[:n]
    ub[:len(rb)] = rb
    assert len(ua) == n
    g = 1.0 if rule.K is None else BR.interp(BR.gains(a, b, rule.hop, rule.K), n, rule.low_sr, rule.native_sr, rule.hop)
    return BR.merge(x, ua, ub, g)
