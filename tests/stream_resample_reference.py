"""TEST INFRASTRUCTURE ONLY -- numpy float64 restatement of the rule by which audio_io.StreamResampler resamples a stream
that arrives in chunks (csrc/stream_resample.hip), on top of oracle.wave_io (resampy's `resample_f`, `kaiser_best`).

Notation of oracle.wave_io.resample_f: ratio = target / orig, scale = min(1, ratio), index_step = int(scale * num_table), nwin =
the length of the half window, time(t) = the running f64 sum of 1 / ratio, n(t) = floor(time(t)).  R = nwin // index_step: the
left wing of output t reads x[n - i] for i < min(n + 1, (nwin - offset) // index_step) and the right wing x[n + 1 + k] for
k < min(n_in - n - 1, (nwin - offset') // index_step); both offsets are >= 0, so neither wing reads more than R samples.

Finality.  Output t depends on the signal's length n_in only through the right wing's bound n_in - n - 1.  With n_recv samples
received, every t with n(t) + 1 + R <= n_recv has n_recv - n - 1 >= R >= (nwin - offset') // index_step: the bound does not
bind, for n_in = n_recv or any longer signal, so the value is final.  Such a t is below int(n_total * ratio), resampy's output
count, for every n_total >= n_recv.  Both facts are asserted at every step.

Retained samples.  T = ready(n_recv) outputs are final; a later output t >= T reads no sample below n(t) - (R - 1)
>= n(T) - (R - 1), so base = max(n(T) - (R - 1), 0) is the first sample still needed and pending = n_recv - base.
Bound: T is not final, so n(T) + 1 + R > n_recv, i.e. n(T) >= n_recv - R, hence base >= n_recv - 2 R + 1 and
    pending <= 2 R - 1
(where base = 0 because n(T) <= R - 1, n_recv <= n(T) + R <= 2 R - 1 as well).  PENDING_BOUND states it; it is exact: a stream
whose n(T) equals n_recv - R attains it.

Close.  With the length n_total known the remaining outputs are [T, n_out), n_out = ceil(n_total * ratio) (fix=True) or
int(n_total * ratio), computed with n_in = n_total; those at or past n_valid = int(n_total * ratio) are zero (librosa's
fix_length).  int(n_total * ratio) < 1 is refused as resampy refuses it."""
import numpy as np

from oracle import wave_io as owio

RATE_PAIRS = [(44100, 14000), (48000, 14000), (16000, 14000), (8000, 14000), (14000, 16000), (14000, 48000), (14000, 44100)]


class Rule:
    def __init__(self, orig_sr, target_sr):
        self.orig_sr, self.target_sr = orig_sr, target_sr
        self.ratio = float(target_sr) / orig_sr
        win, self.num_table = owio.sinc_window()
        self.win = win * self.ratio if self.ratio < 1 else win          # as oracle.wave_io.resample hands it to resample_f
        self.delta = np.zeros_like(self.win)
        self.delta[:-1] = np.diff(self.win)
        self.scale = min(1.0, self.ratio)
        self.index_step = int(self.scale * self.num_table)
        self.nwin = self.win.shape[0]
        self.R = self.nwin // self.index_step
        self.PENDING_BOUND = 2 * self.R - 1
        self._time = np.zeros(1)

    def time(self, n):
        """time(0 .. n - 1): resample_f's register, a literal np.cumsum of 1 / ratio (kept and grown on demand)."""
        if n > len(self._time):
            n_have = max(n, 2 * len(self._time))
            self._time = np.concatenate([[0.0], np.cumsum(np.full(n_have - 1, 1.0 / self.ratio))])
        return self._time[:n]

    def ready(self, n_recv):
        """(T, base): the number of final outputs after n_recv samples, and the first sample a later output reads."""
        time = self.time(int(n_recv * self.ratio) + 3)              # reaches past n_recv
        assert time[-1] >= n_recv
        # time increases, so the final outputs are a prefix: n(t) + 1 + R <= n_recv  <=>  time(t) < n_recv - R
        T = int(np.searchsorted(time, n_recv - self.R, side="left")) if n_recv > self.R else 0
        n = time[max(T - 1, 0):T + 1].astype(np.int64)
        assert (T == 0 or n[0] + 1 + self.R <= n_recv) and n[-1] + 1 + self.R > n_recv
        assert T <= int(n_recv * self.ratio)                        # every final t is an output of any n_total >= n_recv
        return T, max(int(n[-1]) - (self.R - 1), 0)

    def outputs(self, x, n_in, t_lo, t_hi):
        """Outputs [t_lo, t_hi) of resample_f(x[:n_in]): its statements, for a range of t (every output keeps the loop's tap
        order).  The CPU test checks outputs(x, len(x), 0, n_out) == oracle.wave_io.resample_f(x) exactly.  Also returns
        whether no right wing was cut short by n_in (the finality of the range)."""
        x = np.asarray(x, dtype=np.float64)
        time = self.time(max(t_hi, 1))[t_lo:t_hi]
        n = time.astype(np.int64)
        y = np.zeros(max(t_hi - t_lo, 0))
        if not len(y):
            return y, True
        frac = self.scale * (time - n)
        index_frac = frac * self.num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        i_max = np.minimum(n + 1, (self.nwin - offset) // self.index_step)
        for i in range(int(i_max.max())):
            live = i < i_max
            o = np.where(live, offset + i * self.index_step, 0)
            weight = self.win[o] + eta * self.delta[o]
            y += np.where(live, weight * x[np.where(live, n - i, 0)], 0.0)
        frac = self.scale - frac
        index_frac = frac * self.num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        lim = (self.nwin - offset) // self.index_step
        k_max = np.minimum(n_in - n - 1, lim)
        for k in range(max(int(k_max.max()), 0)):
            live = k < k_max
            o = np.where(live, offset + k * self.index_step, 0)
            weight = self.win[o] + eta * self.delta[o]
            y += np.where(live, weight * x[np.where(live, n + k + 1, 0)], 0.0)
        return y, bool(np.all(lim <= n_in - n - 1))

    def stream(self, x, chunk_sizes, fix=True):
        """x fed in chunks of `chunk_sizes` (they sum to len(x)), then closed -> (the emitted pieces, one per chunk and one for the
        close; the largest number of pending samples after a step).  Asserts the two facts and the pending bound at every step."""
        x = np.asarray(x, dtype=np.float64)
        assert sum(chunk_sizes) == len(x)
        n_recv = T = 0
        pieces, most = [], 0
        for c in chunk_sizes:
            n_recv += int(c)
            T_new, base = self.ready(n_recv)
            assert T_new >= T
            y, final = self.outputs(x, n_recv, T, T_new)            # x[:n_recv] is all a final output reads
            assert final
            pieces.append(y)
            T = T_new
            assert 0 <= n_recv - base <= self.PENDING_BOUND, (n_recv, base, self.PENDING_BOUND)
            most = max(most, n_recv - base)
        n_valid = int(n_recv * self.ratio)
        if n_valid < 1:
            raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (n_recv, self.orig_sr, self.target_sr))
        n_out = int(np.ceil(n_recv * self.ratio)) if fix else n_valid
        assert T <= n_valid
        y, _ = self.outputs(x, n_recv, T, n_valid)
        pieces.append(np.concatenate([y, np.zeros(n_out - n_valid)]))
        return pieces, most
