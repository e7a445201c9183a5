"""Host-side glue between the nn.Module mirrors and the C ABI: activation buffers, weight
packing, descriptor filling.  Plumbing only -- all arithmetic on activations happens in the HIP
kernels (include/sos_hip.h)."""
import ctypes as C

import torch

from . import _lib as L
from . import get_precision

BN_EPS = 1e-5


class LaunchProfiler:
    """Optional HIP-event bracket around conv launches on the stream they are enqueued on
    (bench.py's roofline leg).  `only` restricts recording to one launch signature."""

    def __init__(self, only=None):
        self.only = only
        self.records = {}      # signature -> [flops_per_launch, [(start, end), ...]]

    def bracket(self, sig, flops):
        if self.only is not None and sig != self.only:
            return None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(sig, [flops, []])[1].append((s, e))
        s.record()
        return e

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for sig, (flops, evs) in self.records.items():
            ms = [s.elapsed_time(e) for s, e in evs]
            out[sig] = dict(flops=flops, launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms))
        return out


PROFILER = None

# Conv tilings.  By default every process loads the SHIPPED table (tune_table_gfx950.txt, measured once on an MI355X for
# the BASELINE shapes) and uses the deterministic cost-model pick for any other shape: two processes -- or two ranks of
# one data-parallel job -- therefore run identical tilings, i.e. identical summation orders and bit-identical results.
# SOS_CONV_TUNE=1 opts into timing-based autotuning of shapes the table does not hold (sos_conv2d_tune synchronises, so
# it is skipped while a stream capture is in progress); SOS_CONV_TUNE_CACHE=<file> replaces the shipped table and, with
# autotuning on, receives the tuned table at exit (rank 0 only, written atomically).  tools/make_tune_table.py
# regenerates the shipped file.
import os as _os
import threading as _threading

# SOS_LAUNCH_LOG=<file>: one line per conv / weight-gradient launch, in enqueue order: "conv|<signature>" / "wgrad|<signature>".
# profiles/summarize_rocpd.py joins it with the rocprofv3 kernel trace of the same process (the k-th conv-family dispatch is the
# k-th "conv" line), so that the per-kernel table has one row per (kernel, layer signature) and the roofline fraction of the
# dominant SIGNATURE is recomputable from profiles/ (VERDICT r3 #6).  Off by default: no file, no overhead.
_LAUNCH_LOG = None
if _os.environ.get("SOS_LAUNCH_LOG"):
    _LAUNCH_LOG = open(_os.environ["SOS_LAUNCH_LOG"], "a", buffering=1)


def _log_launch(kind, sig, flops):
    _LAUNCH_LOG.write("%s|%s|%.6g\n" % (kind, ",".join(str(v) for v in sig[1:]), flops))

FLATTEN_1X1 = _os.environ.get("SOS_FLATTEN_1X1", "1") != "0"      # A/B switch of the batch-flattened 1x1 layers (conv())
AUTOTUNE = _os.environ.get("SOS_CONV_TUNE", "0") == "1"
if AUTOTUNE and int(_os.environ.get("WORLD_SIZE", "1")) > 1:
    # timing-based tuning is a single-process activity: ranks tuning on their own would pick different tilings -- different
    # summation orders -- during that run.  Tune once with one process, then ship / point every rank at the table.
    import warnings as _warnings
    _warnings.warn("SOS_CONV_TUNE=1 ignored in a multi-process job (WORLD_SIZE > 1): tune with one process and reuse the table")
    AUTOTUNE = False
TUNE_CANDIDATES = int(_os.environ.get("SOS_CONV_TUNE_CANDIDATES", "8"))     # best-ranked tilings of the cost model that get timed
SHIPPED_TUNE_TABLE = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tune_table_gfx950.txt")
SHIPPED_WGRAD_TABLE = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "wgrad_table_gfx950.txt")     # measured weight-gradient plans
_WGRAD_CACHE = _os.environ.get("SOS_WGRAD_TUNE_CACHE")      # user table laid over the shipped one (written at exit when SOS_CONV_TUNE=1)
_tuned = set()
_tune_lock = _threading.Lock()
_TUNE_CACHE = _os.environ.get("SOS_CONV_TUNE_CACHE")
_cache_loaded = set()          # precision-mode libraries whose table has been loaded


def _load_tune_cache():
    which = "fp16" if get_precision() == "fp16" else "bf16"
    if which in _cache_loaded:
        return
    with _tune_lock:
        if which in _cache_loaded:
            return
        # the shipped table first, then the user's cache file of THIS library (X for the bf16 build, X.f16 for the fp16
        # build) laid over it if it exists; a user file this build cannot read is reported and ignored
        user = None if not _TUNE_CACHE else _TUNE_CACHE + ("" if which == "bf16" else ".f16")
        if _os.environ.get("SOS_CONV_TUNE_TABLE", "1") != "0":      # =0: without the shipped table (A/B of the table itself; re-tuning)
            n = L.lib().sos_conv2d_tune_load(SHIPPED_TUNE_TABLE.encode())
            if n < 0:
                raise RuntimeError("sos_conv2d_tune_load: " + (L.lib().sos_last_error() or b"").decode())
        if user and _os.path.exists(user):
            if L.lib().sos_conv2d_tune_load(user.encode()) < 0:
                import warnings
                warnings.warn("SOS_CONV_TUNE_CACHE %s ignored: %s" % (user, (L.lib().sos_last_error() or b"").decode()))
        if AUTOTUNE and user and int(_os.environ.get("RANK", "0")) == 0:
            import atexit
            h = L.lib()
            atexit.register(lambda: h.sos_conv2d_tune_save(user.encode()))
        # the weight-gradient plans: same scheme (one table for both builds: the plans do not depend on the storage type)
        if _os.environ.get("SOS_WGRAD_TUNE_TABLE", "1") != "0":
            if L.lib().sos_wgrad_tune_load(SHIPPED_WGRAD_TABLE.encode()) < 0:
                raise RuntimeError("sos_wgrad_tune_load: " + (L.lib().sos_last_error() or b"").decode())
        # each build keeps its own plan table and saves it at exit: the bf16 build to X, the fp16 build to X.f16 (one path for
        # both made the second save overwrite the first); a build reads X and then its own file over it
        wuser = None if not _WGRAD_CACHE else _WGRAD_CACHE + ("" if which == "bf16" else ".f16")
        for wpath in ([_WGRAD_CACHE] if _WGRAD_CACHE else []) + ([wuser] if wuser and wuser != _WGRAD_CACHE else []):
            if _os.path.exists(wpath) and L.lib().sos_wgrad_tune_load(wpath.encode()) < 0:
                import warnings
                warnings.warn("SOS_WGRAD_TUNE_CACHE %s ignored: %s" % (wpath, (L.lib().sos_last_error() or b"").decode()))
        if AUTOTUNE and wuser and int(_os.environ.get("RANK", "0")) == 0:
            import atexit
            hw = L.lib()
            atexit.register(lambda: hw.sos_wgrad_tune_save(wuser.encode()))
        _cache_loaded.add(which)


def pad_to(x, m):
    return (x + m - 1) // m * m


class Act:
    """bf16 NHWC activation buffer [B, H, W, nseg*cs]; nseg = 3 (hi|hi|lo thirds) in bf16x3
    mode.  `cs` is the per-third channel capacity (multiple of 16)."""

    def __init__(self, B, H, W, cs, x3, device, zero=False):
        self.B, self.H, self.W, self.cs, self.x3 = B, H, W, cs, x3
        self.nseg = 3 if x3 else 1
        alloc = torch.zeros if zero else torch.empty
        self.t = alloc((B, H, W, self.nseg * cs), dtype=act_dtype(), device=device)

    @property
    def dtype_code(self):
        return L.DT_BF16X3 if self.x3 else L.DT_BF16


def is_x3():
    return get_precision() == "bf16x3"


def act_dtype():
    """torch dtype of the 16-bit storage buffers of the current precision mode (torch only allocates them)."""
    return torch.float16 if get_precision() == "fp16" else torch.bfloat16


class GradScale:
    """Loss scale of the fp16 mode for ONE backward pass (include/sos_hip.h, sos_loss_scale): a device pair {S, 1/S}
    chosen from max|g| of the gradients entering the hand-written backward, no host synchronisation.  `mul` is
    multiplied in where f32 gradients become 16-bit, `inv` where parameter gradients leave.  In the bf16 modes both
    are None (bf16 has f32's exponent range)."""

    TARGET = 256.0          # the entering gradients are scaled to max|g| in (128, 256]: 2^8 of headroom, 2^-32 of floor

    def __init__(self, *grads, guard=None):
        self.mul = self.inv = None
        if get_precision() != "fp16":
            return
        gs = [g for g in grads if g is not None]
        if not gs:
            return
        dev = gs[0].device
        buf = torch.zeros(3, dtype=torch.float32, device=dev)
        for g in gs:
            L.check(L.lib().sos_amax_f32(L.ptr(g), g.numel(), L.ptr(buf), L.stream_ptr()), "sos_amax_f32")
        # guard: the model's overflow-guard state (guard_state); its back-off factor lowers the target after overflows
        L.check(L.lib().sos_loss_scale(L.ptr(buf), self.TARGET, L.ptr(buf[1:]), L.ptr(guard), L.stream_ptr()), "sos_loss_scale")
        self.buf, self.mul, self.inv = buf, buf[1:2], buf[2:3]

    def unscale(self, t):
        """In-place 1/S on a small f32 tensor (bias gradients)."""
        if self.inv is not None:
            L.check(L.lib().sos_scale_f32(L.ptr(t), t.numel(), L.ptr(self.inv), L.stream_ptr()), "sos_scale_f32")
        return t


NO_SCALE = GradScale.__new__(GradScale)
NO_SCALE.mul = NO_SCALE.inv = None
_TLS = _threading.local()


class backward_scale:
    """`with backward_scale(g1, g2, ...):` -- the hand-written backward of one network runs inside; wgrad / bn_bwd /
    colsum / pack_grad pick the pass's GradScale up through cur_gs() (thread local: DataParallel-style callers run one
    backward per host thread)."""

    def __init__(self, *grads, guard=None):
        self.gs = GradScale(*grads, guard=guard)

    def __enter__(self):
        self.prev = getattr(_TLS, "gs", NO_SCALE)
        _TLS.gs = self.gs
        return self.gs

    def __exit__(self, *exc):
        _TLS.gs = self.prev
        return False


def cur_gs():
    return getattr(_TLS, "gs", NO_SCALE)


def guard_state(net):
    """The overflow-guard state of a model (include/sos_hip.h, sos_grad_guard): device f32 [SOS_GUARD_FLOATS] =
    {found, back-off, finite steps, skipped steps, scratch}, created on first use on the parameters' device.  The
    backward pass reads its back-off factor (loss scale), the optimizer writes it (FusedAdam.guard)."""
    dev = next(net.parameters()).device
    g = net.__dict__.get("_sos_guard")
    if g is None or g.device != dev:
        g = net.__dict__["_sos_guard"] = torch.zeros(L.GUARD_FLOATS, dtype=torch.float32, device=dev)
    return g


WFOLD = _os.environ.get("SOS_WFOLD", "1") != "0"       # A/B switch: horizontal taps of the 2-channel first layers on the channel axis


def pack_input(x, x3=None, mul=None, wtaps=None, clip_w=None):
    """f32 NCHW module input -> Act with cs = 16 (sos_pack_nchw_to_nhwc); `mul`: optional device scalar (loss scale).
    wtaps = (kw, pad_left, pad_mode): the horizontal taps of the first conv layer folded into the channel axis
    (sos_pack_nchw_wtaps, see wfold_spec); clip_w: int32 device [B], the clips' own widths of a ragged batch."""
    L.require_cuda(x)
    x3 = is_x3() if x3 is None else x3
    x = x.contiguous().float()
    B, Cc, H, W = x.shape
    if wtaps is not None:
        kw, pad_left, pad_mode = wtaps
        a = Act(B, H, W, pad_to(kw * Cc, 16), x3, x.device)
        L.check(L.lib().sos_pack_nchw_wtaps(L.ptr(x), B, Cc, H, W, kw, pad_left, pad_mode, L.ptr(clip_w), L.ptr(a.t),
                                            a.nseg * a.cs, a.dtype_code, L.ptr(mul), L.stream_ptr()), "sos_pack_nchw_wtaps")
        return a
    a = Act(B, H, W, pad_to(Cc, 16), x3, x.device)
    L.check(L.lib().sos_pack_nchw_to_nhwc(L.ptr(x), B, Cc, H, W, L.ptr(a.t), a.nseg * a.cs, a.dtype_code,
                                          L.ptr(mul), L.stream_ptr()), "sos_pack_nchw_to_nhwc")
    return a


def wfold_spec(conv, pad_left, pad_mode):
    """A first layer whose input is the 2-channel module input (Conv2d(2, nf, (1,7)) of the encoders, M1/networks.py:120-128 /
    M2/networks.py:72-80; DownConvBlock(2, 64, 5, 1) of the U-Net, M2/networks.py:158,165): on the MFMA kernels a tap contracts
    16 stored channels of which 2 are real.  With the kw horizontal taps folded into the channel axis by the boundary pack
    (sos_pack_nchw_wtaps: stored channel t*I + c = x[c][h][w + t - pad_left]) the layer is a kh x 1 conv over kw*I real channels
    with w'[o][t*I + c][a][0] = w[o][c][a][t]: 14 (1x7) or 10 (5x5) of 16 channels real, 1/kw of the taps -- forward conv and
    weight gradient alike.  Returns None when the layer does not qualify, else dict(kw, I, wtaps, fold(w), unfold(dw'))."""
    O, I, kh, kw = conv.weight.shape
    if (not WFOLD or kw < 2 or kw * I > 16 or conv.dilation[1] != 1 or conv.stride[1] != 1 or conv.stride[0] != 1):
        return None
    return dict(kw=kw, I=I, wtaps=(kw, pad_left, pad_mode),
                fold=lambda w: w.permute(0, 3, 1, 2).reshape(O, kw * I, kh, 1),
                unfold=lambda dw: dw.reshape(O, kw, I, kh).permute(0, 2, 3, 1).contiguous())


def pack_weight(w, cin_store, x3, in_perm=None):
    """Conv weight (O, I, kh, kw) f32 -> 16-bit [kh*kw][O_pad][nseg*cin_store].  In bf16x3 mode the
    K axis is [w_hi | w_lo | w_hi], matching activations stored [x_hi | x_hi | x_lo], so one MFMA
    pass computes x_hi*w_hi + x_hi*w_lo + x_lo*w_hi.  `in_perm` reorders input channels (concat
    buffers whose parts are stored in a different order than torch.cat's).
    `w` may be a zero-argument callable returning the (layout-derived) weight: under a PackRecorder in replay mode
    (the per-step refresh of a training plan) it is not even evaluated -- the packed tensor was refreshed by
    sos_gather_pack_multi."""
    rec = getattr(_TLS, "pack_rec", None)
    if rec is not None and rec.mode == "replay":
        return rec.next_out()
    if callable(w):
        w = w()
    O, I, kh, kw = w.shape
    w = w.detach().float()
    if in_perm is not None:
        w = w[:, in_perm]
    wp = w.permute(2, 3, 0, 1).reshape(kh * kw, O, I)
    Op = pad_to(O, 32)
    full = torch.zeros((kh * kw, Op, cin_store), dtype=torch.float32, device=w.device)
    full[:, :O, :I] = wp
    if rec is not None and rec.mode == "index":
        # parameters hold their own (1-based) element ids: `full` is the relocation map; low parts carry a minus sign
        rec.idx.append(torch.cat([full, -full, full], dim=2).contiguous() if x3 else full.contiguous())
        return full
    hi = full.to(act_dtype())
    if not x3:
        out = hi.contiguous()
    else:
        lo = (full - hi.float()).to(act_dtype())
        out = torch.cat([hi, lo, hi], dim=2).contiguous()
    if rec is not None and rec.mode == "value":
        rec.outs.append(out)
    return out


class PackRecorder:
    """Turns the per-step re-packing of a plan's weights (~10 torch kernels per packed tensor, ~1000 per training step)
    into one sos_gather_pack_multi launch.  Built once per (module, precision, parameter storage): the plan builder runs
    a second time with every parameter temporarily holding its own element ids, so each pack_weight call yields the
    relocation map of its output; the maps become tables of absolute source addresses.  Every map is VERIFIED against
    the value-built tensor before it is trusted (a packed tensor that is not a pure relocation of parameter elements
    disables the recorder, and the plan is simply rebuilt by torch as before)."""

    ENABLED = _os.environ.get("SOS_PACK_GATHER", "1") != "0"

    def __init__(self, module, build):
        self.mode, self.outs, self.idx, self.k, self.ok = "value", [], [], 0, False
        params = [p for p in module.parameters()]
        prev = getattr(_TLS, "pack_rec", None)
        _TLS.pack_rec = self
        try:
            self.plan = build()
            if not self.ENABLED or not self.outs or sum(p.numel() for p in params) >= (1 << 24):
                return                                  # ids must be exact in float32
            saved, start = [], 0
            starts = []
            for p in params:
                saved.append(p.data)
                starts.append(start)
                p.data = torch.arange(start + 1, start + 1 + p.numel(), dtype=torch.float32, device=p.device).reshape(p.shape)
                start += p.numel()
            self.mode = "index"
            try:
                build()
            finally:
                for p, d in zip(params, saved):
                    p.data = d
        finally:
            _TLS.pack_rec = prev
            self.mode = "idle"
        if len(self.idx) != len(self.outs) or any(i.shape != o.shape for i, o in zip(self.idx, self.outs)):
            return
        dev = self.outs[0].device
        ptrs = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
        st = torch.tensor(starts, dtype=torch.int64, device=dev)
        tabs, rows, chunks = [], [], []
        for ei, (ids, out) in enumerate(zip(self.idx, self.outs)):
            a = ids.reshape(-1).abs().round().to(torch.int64)
            pi = torch.bucketize(a, st, right=False) - 1                    # ids of parameter k lie in (start_k, start_k + n_k]
            pi = pi.clamp_(min=0)
            addr = ptrs[pi] + 4 * (a - 1 - st[pi])
            addr = torch.where(a == 0, torch.zeros_like(addr), torch.where(ids.reshape(-1) < 0, -addr, addr)).contiguous()
            tabs.append(addr)
            rows.append([addr.data_ptr(), out.data_ptr(), out.numel()])
            chunks += [[ei, c] for c in range((out.numel() + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK)]
        self.idx = None
        self.tabs = tabs
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self.n, self.nchunks = len(rows), len(chunks)
        # trust, but verify: replay into scratch copies and compare with what torch built
        keep = [o.clone() for o in self.outs]
        for o in self.outs:
            o.zero_()
        self.refresh()
        self.ok = all(torch.equal(a, b) for a, b in zip(self.outs, keep))
        if not self.ok:
            for o, kcopy in zip(self.outs, keep):
                o.copy_(kcopy)

    def refresh(self):
        L.check(L.lib().sos_gather_pack_multi(L.ptr(self.table), self.n, L.ptr(self.chunks), self.nchunks, L.stream_ptr()),
                "sos_gather_pack_multi")

    def next_out(self):
        o = self.outs[self.k]
        self.k += 1
        return o

    def replay(self, build):
        """Refresh every packed weight (one launch) and rebuild the plan around them (the builder's other, small pieces
        -- bias vectors, the LSTM's fragment pack -- are recomputed as usual)."""
        self.refresh()
        prev = getattr(_TLS, "pack_rec", None)
        _TLS.pack_rec, self.mode, self.k = self, "replay", 0
        try:
            plan = build()
        finally:
            _TLS.pack_rec, self.mode = prev, "idle"
        if self.k != len(self.outs):
            raise RuntimeError("PackRecorder: the plan builder changed its pack_weight sequence")
        return plan


def pad_vec(v, n, fill=0.0):
    out = torch.full((n,), fill, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.detach().float().reshape(-1)
    return out


def fold_bn(bn, cout_pad):
    """Eval-mode BatchNorm2d as per-channel scale/shift for the conv epilogue."""
    scale = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    return pad_vec(scale, cout_pad, 1.0), pad_vec(shift, cout_pad, 0.0)


def conv(src, cin_off, cin, wgt, kh, kw, cout, scale, shift, act, *, out, out_dtype, sb, sh, sw, sc,
         Ho, Wo, c_off=0, cout_store=None, third=0, stride=1, dil=(1, 1), pad=(0, 0), pad_mode=L.PAD_ZERO,
         slope=None, w_gather=None, out_elem_offset=0, in_dims=None, accumulate=False, stats_c=0, wl_tab=None,
         wo_tab=None, wg_stride=0, valid_cols=None, temporal=None, fold=None, in_bn=None):
    """Fill a sos_conv_desc and enqueue sos_conv2d_fwd.  `src` is an Act (or a (tensor,B,H,W,cs,nseg)
    view described by in_dims).  stats_c > 0: also return the fused BatchNorm partial sums of the first stats_c
    output channels as (partial [2][stats_c][tiles], tiles) for sos_bn_finalize.  temporal = (frames per clip, kt): the
    B images are clips of consecutive frames and the contraction also runs over kt neighbouring frames (Conv3d with
    temporal stride 1, padding (kt - 1) // 2); `cin` stays the channels of ONE frame.  fold = (padded scratch Act, pad, H, W,
    sy, oy, sx, ox): reflection-pad fold of the output (sos_conv_desc.fold_*): `out` / sb / sw then describe the dense
    [B][H][W] gradient tensor the interior cells go to."""
    d = L.ConvDesc()
    if in_dims is None:
        t, B, H, W, cs, nseg = src.t, src.B, src.H, src.W, src.cs, src.nseg
    else:
        t, B, H, W, cs, nseg = in_dims
    # 1x1 layers over single-row images (Linear layers, LSTM input projections: H = 1, W = T frames): the batch is one long
    # row -- full 256-pixel tiles instead of one ragged tile per clip (T = 178: 70 % of a tile, the detector's T = 60: 23 %)
    Bp, Wop = B, Wo                       # (the profiler's signature keeps the layer's own dimensions)
    if (FLATTEN_1X1 and kh == 1 and kw == 1 and stride == 1 and pad == (0, 0) and H == 1 and Ho == 1 and Wo == W and B > 1
            and w_gather is None and wl_tab is None and temporal is None and fold is None and not stats_c and sb == Wo * sw
            and B * W * nseg * cs * 2 < 0xfff00000 and B * Wo * sw < 0x7ffffff0):     # (input bytes and output offsets stay 32-bit)
        B, W, Wo = 1, B * W, B * Wo
    d.in_ = t.data_ptr()
    d.B, d.H, d.W = B, H, W
    d.in_cs = nseg * cs
    d.cin_off, d.cin, d.in_nseg, d.in_seg_stride = cin_off, cin, nseg, cs
    if w_gather is not None:
        d.w_gather = w_gather.data_ptr()
        d.Wl = w_gather.numel()
    else:
        d.w_gather = None
        d.Wl = W
    d.wgt = wgt.data_ptr()
    d.kh, d.kw, d.cout, d.cout_pad = kh, kw, cout, wgt.shape[1]
    d.stride, d.dil_h, d.dil_w = stride, dil[0], dil[1]
    d.pad_top, d.pad_left, d.pad_mode = pad[0], pad[1], pad_mode
    d.Ho, d.Wo = Ho, Wo
    esize = 4 if out_dtype == L.DT_F32 else 2
    d.out = out.data_ptr() + out_elem_offset * esize
    d.out_dtype = out_dtype
    d.out_sb, d.out_sh, d.out_sw, d.out_sc = sb, sh, sw, sc
    d.out_c_off = c_off
    d.cout_store = cout if cout_store is None else cout_store
    d.out_third = third
    d.scale, d.shift = (scale.data_ptr(), shift.data_ptr()) if scale is not None else (None, None)
    d.act = act
    d.act_param = slope.data_ptr() if slope is not None else None
    d.accumulate = 1 if accumulate else 0
    if temporal is not None and temporal[1] > 1:
        d.t_frames, d.t_taps, d.t_pad = temporal[0], temporal[1], (temporal[1] - 1) // 2
    if wl_tab is not None:                # ragged batch: per-image logical input width / valid output width (sos_hip.h)
        d.wl_tab, d.wo_tab, d.w_gather_stride = wl_tab.data_ptr(), wo_tab.data_ptr(), wg_stride
    if in_bn is not None:                 # (scale, shift) f32 [cin] of the producer's BatchNorm: `src` is its RAW output (sos_conv_desc.in_scale)
        d.in_scale, d.in_shift = in_bn[0].data_ptr(), in_bn[1].data_ptr()
    if fold is not None:
        fa, fp, fH, fW, fsy, foy, fsx, fox = fold
        d.fold_pad_out, d.fold_pad, d.fold_H, d.fold_W = fa.t.data_ptr(), fp, fH, fW
        d.fold_sy, d.fold_oy, d.fold_sx, d.fold_ox = fsy, foy, fsx, fox
        d.fold_row, d.fold_third = fa.nseg * fa.cs, fa.cs
    _load_tune_cache()
    if AUTOTUNE:
        # (folded data-gradient launches are tuned like any other shape: with the fused fold -- the default -- the plain
        # padded-domain launch they used to share a tiling with no longer happens)
        key = (B, H, W, d.Wl, cin, d.in_nseg, d.cout_pad, cout, kh, kw, stride, dil, Ho, Wo, out_dtype, sc == 1, pad_mode,
               w_gather is not None, d.t_taps)
        if key not in _tuned and not torch.cuda.is_current_stream_capturing():
            _tuned.add(key)
            if accumulate or fold is not None:
                # the tuner launches the kernel many times: never let it accumulate into (or store interior cells over) the
                # real gradient buffer -- tune a non-accumulating copy of the descriptor on scratch output
                scratch = torch.empty_like(out)
                real_out, real_acc = d.out, d.accumulate
                d.out = scratch.data_ptr() + out_elem_offset * esize
                d.accumulate = 0
                L.check(L.lib().sos_conv2d_tune(C.byref(d), TUNE_CANDIDATES, 3, None, L.stream_ptr()), "sos_conv2d_tune")
                d.out, d.accumulate = real_out, real_acc
            else:
                L.check(L.lib().sos_conv2d_tune(C.byref(d), TUNE_CANDIDATES, 3, None, L.stream_ptr()), "sos_conv2d_tune")
    end = None
    if PROFILER is not None or _LAUNCH_LOG is not None:
        # ragged batches: only the clips' own columns are algorithmic work (valid_cols = their sum)
        cols = Bp * Wop if valid_cols is None else valid_cols
        kin = d.in_nseg * max(1, d.t_taps) * cin
        sig = ("conv", kh, kw, dil[0], dil[1], stride, kin, cout, Bp, Ho, Wop) + (() if valid_cols is None else ("ragged", cols))
        if _LAUNCH_LOG is not None:
            _log_launch("conv", sig, 2.0 * Ho * cols * cout * kin * kh * kw)
        if PROFILER is not None:
            end = PROFILER.bracket(sig, 2.0 * Ho * cols * cout * kin * kh * kw)
    stats = None
    if stats_c:
        tiles = L.lib().sos_conv2d_tile_count(C.byref(d))
        if tiles < 1:
            raise RuntimeError("sos_conv2d_tile_count: " + (L.lib().sos_last_error() or b"").decode())
        stats = (torch.empty((2, stats_c, tiles), dtype=torch.float32, device=out.device), int(tiles))
        d.stats, d.stats_c = stats[0].data_ptr(), stats_c
    L.check(L.lib().sos_conv2d_fwd(C.byref(d), L.stream_ptr()), "sos_conv2d_fwd")
    if end is not None:
        end.record()
    return stats


def conv_to_phase(src, cin_off, cin, wgt, kh, kw, cout, scale, shift, act, dst, s, rh, rw, c_off=0, cout_store=None, **kw_):
    """Conv whose output pixel (i, j) is pixel (s * i + rh, s * j + rw) of (a channel slice of) a dense NHWC Act: phase
    (rh, rw) of its stride-s grid.  The one place that writes this geometry; Ho / Wo (the phase's own size) are the caller's."""
    row = dst.nseg * dst.cs
    return conv(src, cin_off, cin, wgt, kh, kw, cout, scale, shift, act, out=dst.t, out_dtype=dst.dtype_code,
                sb=dst.H * dst.W * row, sh=s * dst.W * row, sw=s * row, sc=1, c_off=c_off,
                cout_store=cout if cout_store is None else cout_store, third=dst.cs,
                out_elem_offset=(rh * dst.W + rw) * row, **kw_)


def conv_to_act(src, cin_off, cin, wgt, kh, kw, cout, scale, shift, act, dst, c_off=0, cout_store=None, **kw_):
    """Conv whose output is (a channel slice of) a dense NHWC Act."""
    return conv_to_phase(src, cin_off, cin, wgt, kh, kw, cout, scale, shift, act, dst, 1, 0, 0, c_off, cout_store, **kw_)


def lstm_gate_perm(H, device):
    """Row permutation torch order (dir, gate q, unit j) -> the kernels' gate-interleaved order (dir, j, q):
    new[n] = old[perm[n]]; inv undoes it (old[o] = new[inv[o]])."""
    n = torch.arange(8 * H, device=device)
    d, r = n // (4 * H), n % (4 * H)
    perm = d * 4 * H + (r % 4) * H + r // 4
    inv = torch.empty_like(perm)
    inv[perm] = n
    return perm, inv


def lstm_pack(lstm_mod, x3):
    """W_hh of both directions -> the MFMA fragment arrays of the recurrent kernels (sos_lstm_pack_whh);
    the lo arrays exist only in bf16x3 mode."""
    H = lstm_mod.hidden_size
    whh = torch.stack([lstm_mod.weight_hh_l0.detach(), lstm_mod.weight_hh_l0_reverse.detach()]).float().contiguous()
    L.require_cuda(whh)
    nf, nb = L.lib().sos_lstm_pack_bytes(H, 0), L.lib().sos_lstm_pack_bytes(H, 1)
    if nf < 0:
        raise RuntimeError(f"LSTM hidden size {H} not supported (multiple of 4, <= 256)")
    mk = lambda n: torch.empty(n // 2, dtype=torch.bfloat16, device=whh.device)   # noqa: E731
    pk = dict(fh=mk(nf), bh=mk(nb), fl=mk(nf) if x3 else None, bl=mk(nb) if x3 else None)
    L.check(L.lib().sos_lstm_pack_whh(L.ptr(whh), H, L.ptr(pk["fh"]), L.ptr(pk["fl"]), L.ptr(pk["bh"]), L.ptr(pk["bl"]),
                                      L.stream_ptr()), "sos_lstm_pack_whh")
    return pk


def lstm(xproj, wpk, B, T, H, out_act, save_gates=None, save_c=None, lengths=None):
    """Recurrent part (sos_lstm_bidir_fwd); wpk from lstm_pack; out_act: Act [B,1,T,cs>=2H] pre-zeroed; lengths:
    optional int32 device [B] (ragged batch)."""
    L.check(L.lib().sos_lstm_bidir_fwd(L.ptr(xproj), L.ptr(wpk["fh"]), L.ptr(wpk["fl"]), B, T, H, L.ptr(out_act.t),
                                       out_act.nseg * out_act.cs, out_act.dtype_code, out_act.cs,
                                       L.ptr(save_gates), L.ptr(save_c), L.ptr(lengths), L.stream_ptr()), "sos_lstm_bidir_fwd")


def upload(values, dtype, device):
    """Small host table -> device WITHOUT blocking the host: staged in pinned memory and copied asynchronously on the
    current stream (torch.tensor(..., device=) / .to(device) from pageable memory wait until the stream has drained --
    24 such waits made the ragged pipeline's host time 364 of its 418 ms).  torch's pinned-memory allocator keeps the staging
    block alive until the copy has run."""
    h = torch.as_tensor(values, dtype=dtype)
    if torch.cuda.is_current_stream_capturing():
        return h.to(device)
    hp = torch.empty(h.shape, dtype=dtype, pin_memory=True)
    hp.copy_(h)
    return hp.to(device, non_blocking=True)


class Ragged:
    """Per-clip widths of a ragged batch (BASELINE configs[3]: clips of different lengths in one launch; buffers are
    sized for the longest clip, every kernel takes the clips' own widths from small device tables).  `T` = STFT frames
    per clip; level(k) = width after k stride-2 blocks ((w + 1) // 2 each, M2/networks.py:158-176)."""

    def __init__(self, T, device, n_vframes=None, n_samples=None):
        self.T = [int(t) for t in T]
        self.device = device
        self.n_vframes = None if n_vframes is None else [int(n) for n in n_vframes]
        self.n_samples = None if n_samples is None else [int(n) for n in n_samples]
        self._tabs = {}

    def widths(self, level):
        w = self.T
        for _ in range(level):
            w = [(x + 1) // 2 for x in w]
        return w

    def tab(self, widths):
        key = tuple(int(x) for x in widths)
        t = self._tabs.get(key)
        if t is None:
            t = self._tabs[key] = upload(key, torch.int32, self.device)
        return t

    def level(self, k):
        return self.tab(self.widths(k))

    def kw(self, lin, lout=None):
        """conv keyword arguments for a layer reading level `lin` and writing level `lout`."""
        lout = lin if lout is None else lout
        return dict(wl_tab=self.level(lin), wo_tab=self.level(lout), valid_cols=sum(self.widths(lout)))


class MaskedRagged(Ragged):
    """A ragged geometry restricted ON THE DEVICE to the clips a 16-bit detector pass marked (sos_logit_band_mark): the host-side
    lists are the base geometry's, every device width table is the base table where mark[b] = 1 and 0 elsewhere, so a launch
    sequence over this geometry computes the marked clips only (tiles of a zero-width clip exit at once; the BiLSTM idles on a
    zero-length clip) and no selection ever reaches the host.  Built by mask_ragged()."""

    def __init__(self, base, mark, tabs):
        super().__init__(base.T, base.device, n_vframes=base.n_vframes, n_samples=base.n_samples)
        self.base, self.mark = base, mark
        self._tabs.update(tabs)
        for k, v in base._tabs.items():           # tables that are not widths (the nearest-resize gather rows) are shared
            if isinstance(k, tuple) and k and isinstance(k[0], str):
                self._tabs.setdefault(k, v)

    def tab(self, widths):
        key = tuple(int(x) for x in widths)
        t = self._tabs.get(key)
        if t is None:                             # a table the mark kernel was not handed: masked by one tiny elementwise launch
            t = self._tabs[key] = self.base.tab(widths) * self.mark
        return t


_band_count = {}


def band_count(device):
    """int32 [2] on `device`: {clips the two-pass detector re-ran in the parity precision, clips it saw} since the process started
    (sos_logit_band_mark accumulates; reading it synchronises -- bench.py does so outside its timed regions)."""
    key = str(device)
    if key not in _band_count:
        _band_count[key] = torch.zeros(2, dtype=torch.int32, device=device)
    return _band_count[key]


def mask_ragged(base, logits, band_rel, width_lists, scale=None):
    """logits f32 (B, n) of a 16-bit detector pass over the geometry `base` -> (MaskedRagged, mark int32 (B,)).  width_lists:
    the per-clip width lists whose device tables the second pass will ask for (masked by the same launch).  scale: optional f32
    (B, n), the per-frame magnitude the pass's logit error is relative to (sos_logit_band_mark)."""
    B, n = logits.shape
    if scale is not None and (scale.shape != logits.shape or scale.dtype != torch.float32 or not scale.is_contiguous()):
        raise ValueError("mask_ragged: scale must be a contiguous float32 tensor of the logits' shape")
    tabs_in = torch.stack([base.tab(w) for w in width_lists]).contiguous()
    tabs_out = torch.empty_like(tabs_in)
    mark = torch.empty(B, dtype=torch.int32, device=logits.device)
    nv = base.tab(base.n_vframes) if base.n_vframes is not None else None
    L.check(L.lib().sos_logit_band_mark(L.ptr(logits), L.ptr(scale), B, n, L.ptr(nv), float(band_rel), L.ptr(tabs_in), L.ptr(tabs_out),
                                        len(width_lists), L.ptr(mark), L.ptr(band_count(logits.device)), L.stream_ptr()),
            "sos_logit_band_mark")
    tabs = {tuple(int(x) for x in w): tabs_out[k] for k, w in enumerate(width_lists)}
    return MaskedRagged(base, mark, tabs), mark


class PlanCache:
    """Packed weights keyed by the parameters' in-place version counters (optimizer steps and
    load_state_dict bump them), the device, the precision mode and the parameters' storage.  When only the VALUES changed
    (an optimizer step) the packed weights are refreshed in place by one gather launch (PackRecorder) instead of being
    rebuilt by torch."""

    def __init__(self, record=False):
        # record=True (training plans: refreshed every optimizer step): PackRecorder.  Its recording pass briefly swaps
        # the parameters' storage, so inference plans -- which DataParallel-style callers may build from several host
        # threads at once, and which are rebuilt only when new weights are loaded -- do not use it.
        self.key = None
        self.plan = None
        self.rec = None
        self.record = record
        self.rec_failed = set()     # bases whose recording did not verify: plain rebuilds from then on

    def get(self, module, build):
        ts = list(module.parameters()) + list(module.buffers())
        base = (get_precision(), str(ts[0].device), tuple(t.data_ptr() for t in ts), tuple(tuple(t.shape) for t in ts))
        key = (base, tuple(t._version for t in ts))
        if key != self.key:
            with torch.no_grad():
                if self.rec is not None and self.rec.ok and self.rec_base == base:
                    self.plan = self.rec.replay(build)
                elif self.record and base not in self.rec_failed:
                    self.rec, self.rec_base = PackRecorder(module, build), base
                    self.plan = self.rec.plan
                    self.rec.plan = None
                    if not self.rec.ok:
                        self.rec_failed.add(base)
                else:
                    self.plan = build()
            self.key = key
            if isinstance(self.plan, dict):
                # a training tape is only valid for the weights its forward pass ran with (the packed tensors are
                # refreshed IN PLACE after an optimizer step): check_tape_weights() compares these in backward
                self.plan["_wver"] = tuple(p._version for p in module.parameters())
        return self.plan


def check_tape_weights(module, tape):
    """Backward of a tape whose forward ran with older weights would silently use the new ones (the packed weights of a
    training plan are refreshed in place by PackRecorder.replay): refuse."""
    want = tape["plan"].get("_wver")
    if want is not None and want != tuple(p._version for p in module.parameters()):
        raise RuntimeError("sos_amd: the parameters changed (optimizer step / load_state_dict) between this forward pass and "
                           "its backward pass; run backward before stepping the optimizer")


# --------------------------------------------------------------------------- training helpers
def view(act, c_off=0, C=None, third_index=None):
    """sos_view of a channel slice of an Act.  third_index selects ONE third of a bf16x3 buffer as
    a plain bf16 view (used by the three-pass wgrad)."""
    v = L.View()
    v.ptr = act.t.data_ptr()
    v.npix = act.B * act.H * act.W
    v.row = act.nseg * act.cs
    v.C = act.cs if C is None else C
    if third_index is None:
        v.c_off, v.x3, v.third = c_off, 1 if act.x3 else 0, act.cs
    else:
        v.c_off, v.x3, v.third = c_off + third_index * act.cs, 0, 0
    return v


def bn_train(raw, c_off, Cn, bn, act, slope, dst, dst_c_off=0, feat=None, stats=None):
    """Training-mode BatchNorm (+activation) of the raw conv output `raw[:, c_off:c_off+C]`:
    stats -> finalize (updates bn.running_* in place like torch) -> apply into `dst`.
    `stats` = (partial, tiles) from the producing conv's fused statistics (engine.conv(stats_c=...)) skips the
    separate statistics pass.  Returns the saved tensors for backward."""
    dev = raw.t.device
    xv = view(raw, c_off, Cn)
    if stats is not None:
        partial, nblk = stats
    else:
        nblk = L.lib().sos_bn_stats_blocks(xv.npix)
        partial = torch.empty((2, Cn, nblk), dtype=torch.float32, device=dev)
        L.check(L.lib().sos_bn_stats(C.byref(xv), L.ptr(partial), L.stream_ptr()), "sos_bn_stats")
    scale = torch.empty(Cn, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    mean = torch.empty_like(scale)
    invstd = torch.empty_like(scale)
    L.check(L.lib().sos_bn_finalize(L.ptr(partial), nblk, Cn, xv.npix, L.ptr(bn.weight), L.ptr(bn.bias), float(bn.eps),
                                    float(bn.momentum), L.ptr(bn.running_mean), L.ptr(bn.running_var),
                                    L.ptr(bn.num_batches_tracked), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                                    L.stream_ptr()), "sos_bn_finalize")
    for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
        bump_version(t)
    bn_apply(xv, scale, shift, act, slope, dst, dst_c_off, Cn, feat)
    return dict(scale=scale, shift=shift, mean=mean, invstd=invstd)


def bump_version(t):
    """Our kernels write parameters / buffers through raw pointers; tell torch (and the packed-weight
    caches keyed on `_version`) that the tensor changed."""
    try:
        torch.autograd.graph.increment_version(t)
    except AttributeError:       # older torch: a no-op in-place op does the same
        with torch.no_grad():
            t.add_(0)


def bn_apply(xv, scale, shift, act, slope, dst, dst_c_off, C, feat=None):
    import ctypes
    if feat is None:
        yv = view(dst, dst_c_off, C)
        L.check(L.lib().sos_bn_act_apply(ctypes.byref(xv), L.ptr(scale), L.ptr(shift), act, L.ptr(slope), ctypes.byref(yv),
                                         0, 0, 0, None, L.stream_ptr()), "sos_bn_act_apply")
    else:
        # feat = dict(t=feature tensor, row, third, c_off, H, W, Wo, gather, x3)
        yv = L.View()
        yv.ptr, yv.npix, yv.row, yv.c_off, yv.C = feat["t"].data_ptr(), 1, feat["row"], feat["c_off"], C
        yv.x3, yv.third = (1 if feat["x3"] else 0), feat["third"]
        L.check(L.lib().sos_bn_act_apply(ctypes.byref(xv), L.ptr(scale), L.ptr(shift), act, L.ptr(slope), ctypes.byref(yv),
                                         feat["H"], feat["W"], feat["Wo"], L.ptr(feat.get("gather")), L.stream_ptr()),
                "sos_bn_act_apply(feat)")


_wg_ws = {}
# Deferred reduction of the weight gradients (round 4, ABI 8).  A weight gradient is two launches: the MFMA kernel that leaves one
# partial sum per pixel split, and a small HBM-bound reduce of those partials into dw -- which nobody needs before the optimizer.
# With defer=True the reduce runs on a side stream behind an event (it then overlaps the next layers' MFMA kernels instead of
# sitting between them: 72 launches, 1.8 ms of a 117 ms step), the partial sums live in a ring of workspaces (a slot is reused only
# after the reduce that read it), and wgrad_join() makes the consuming stream wait before the gradients are handed on.
# Same kernels, same summation order: bit-identical gradients (tests/test_gpu_agent.py).  MEASURED SLOWER: 539.9 -> 535.7 utt/s
# (-0.8 %, same box, arms alternating) -- the trailing reduces take bandwidth and CUs from the kernels they run beside and the
# two events per layer are not free; the launch gap they were meant to close is ~2 us.  Off by default (SOS_WGRAD_DEFER=1 opts in).
WGRAD_DEFER = _os.environ.get("SOS_WGRAD_DEFER", "0") == "1"
_WG_RING_SLOTS = 4


class _WgState(_threading.local):
    """Per HOST THREAD (DataParallel-style callers run one backward per thread; an inner scope exit on one thread must
    not skip the join another thread's gradients need): ring = origin stream -> dict(slots=[[tensor, event], ...], nxt, side),
    pending = reduce stream -> event of its last reduce not yet joined, scope > 0 inside deferred_reductions()."""

    def __init__(self):
        self.ring, self.pending, self.scope = {}, {}, 0


_wg = _WgState()
WG_STATS = {"deferred": 0, "joined": 0}      # process-wide counters (diagnostics / tests: the autograd engine runs backward on its own thread)


class deferred_reductions:
    """`with deferred_reductions():` around a model's whole backward pass: weight gradients marked defer=True reduce on the side
    stream, and leaving the scope joins them.  Outside the scope every wgrad is complete on the calling stream when it returns
    (what a caller that reads a gradient right after one backward function -- the tests do -- relies on)."""

    def __enter__(self):
        _wg.scope += 1
        return self

    def __exit__(self, *exc):
        _wg.scope -= 1
        if _wg.scope == 0:
            wgrad_join()


def wgrad_join():
    """The current stream waits for every deferred weight-gradient reduce launched so far (call before the gradients are used)."""
    if _wg.pending:
        cur = torch.cuda.current_stream()
        for ev in _wg.pending.values():
            cur.wait_event(ev)
        WG_STATS["joined"] += len(_wg.pending)
        _wg.pending.clear()


def wgrad(g, g_off, M, x, x_off, N, kh, kw, dw, *, stride=1, dil=(1, 1), pad=(0, 0), pad_mode=L.PAD_ZERO,
          accumulate=False, scale=1.0, temporal=None, defer=False):
    """dw[m][n][a][b] (+)= scale * sum_p G[p][m] X[p*stride + (a,b)*dil - pad][n] (sos_conv2d_wgrad).
    g, x: Act.  In bf16x3 mode the product (g_hi+g_lo)(x_hi+x_lo) is taken as hi*hi + hi*lo + lo*hi
    with three accumulating passes over the thirds.  temporal = (frames per clip, kt, channels per frame): column
    n = dt * channels + c pairs image b of G with channel c of frame b + dt - (kt - 1) // 2 of X (sos_wgrad_desc)."""
    import ctypes
    dev = g.t.device
    gs = cur_gs()
    passes = [(0, 0)] if not g.x3 else [(0, 0), (0, 2), (2, 0)]
    first = True
    for gt, xt in passes:
        d = L.WgradDesc()
        d.g, d.B, d.Hg, d.Wg, d.g_cs, d.g_off = g.t.data_ptr(), g.B, g.H, g.W, g.nseg * g.cs, g_off + gt * g.cs
        d.x, d.Hx, d.Wx, d.x_cs, d.x_off = x.t.data_ptr(), x.H, x.W, x.nseg * x.cs, x_off + xt * x.cs
        d.M, d.N, d.kh, d.kw, d.stride, d.dil_h, d.dil_w = M, N, kh, kw, stride, dil[0], dil[1]
        d.pad_top, d.pad_left, d.pad_mode = pad[0], pad[1], pad_mode
        if temporal is not None and temporal[1] > 1:
            d.t_frames, d.t_taps, d.t_pad, d.t_cin = temporal[0], temporal[1], (temporal[1] - 1) // 2, temporal[2]
        npix = g.B * g.H * g.W
        d.ksplit = 0                               # automatic pixel-range split (one workgroup per CU)
        need = L.lib().sos_wgrad_workspace_bytes(ctypes.byref(d))
        cur_stream = torch.cuda.current_stream(dev)
        key = (str(dev), cur_stream.cuda_stream)     # one workspace per stream: agents may run concurrently
        # (never with autotuning on: _partial and _reduce each derive the launch plan from the plan table, which a tune between
        # the two calls could change -- ADVICE r4; the shipped table is loaded once, before the first launch)
        deferred = defer and WGRAD_DEFER and not AUTOTUNE and _wg.scope > 0 and not torch.cuda.is_current_stream_capturing()
        slot = None
        if deferred:
            ring = _wg.ring.get(key)
            if ring is None:
                ring = _wg.ring[key] = dict(slots=[[None, None] for _ in range(_WG_RING_SLOTS)], nxt=0,
                                            side=torch.cuda.Stream(device=dev))
            slot = ring["slots"][ring["nxt"]]
            ring["nxt"] = (ring["nxt"] + 1) % _WG_RING_SLOTS
            if slot[1] is not None:
                cur_stream.wait_event(slot[1])         # the reduce that last read this workspace
            if slot[0] is None or slot[0].numel() * 4 < need:
                slot[0] = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
            d.partial = slot[0].data_ptr()
        else:
            if key not in _wg_ws or _wg_ws[key].numel() * 4 < need:
                _wg_ws[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
            d.partial = _wg_ws[key].data_ptr()
        d.dw = dw.data_ptr()
        d.accumulate = 1 if (accumulate or not first) else 0
        d.scale = scale
        d.scale_dev = gs.inv.data_ptr() if gs.inv is not None else None
        _load_tune_cache()
        if AUTOTUNE and not torch.cuda.is_current_stream_capturing():
            tkey = ("wgrad", g.B, g.H, g.W, x.H, x.W, M, N, kh, kw, stride, dil, d.t_taps)
            if tkey not in _tuned:
                _tuned.add(tkey)
                scratch = torch.empty_like(dw)             # the tuner launches the kernel many times: never into the real gradient
                d.dw, d.accumulate = scratch.data_ptr(), 0
                L.check(L.lib().sos_wgrad_tune(ctypes.byref(d), 3, None, L.stream_ptr()), "sos_wgrad_tune")
                d.dw, d.accumulate = dw.data_ptr(), 1 if (accumulate or not first) else 0
        end = None
        if PROFILER is not None or _LAUNCH_LOG is not None:
            sig = ("wgrad", kh, kw, dil[0], dil[1], stride, M, N, g.B, g.H, g.W)
            if _LAUNCH_LOG is not None:
                _log_launch("wgrad", sig, 2.0 * g.B * g.H * g.W * M * N * kh * kw)
            if PROFILER is not None:
                end = PROFILER.bracket(sig, 2.0 * g.B * g.H * g.W * M * N * kh * kw)
        if deferred:
            side = ring["side"]
            L.check(L.lib().sos_conv2d_wgrad_partial(ctypes.byref(d), L.stream_ptr()), "sos_conv2d_wgrad_partial")
            if end is not None:
                end.record()
            done = torch.cuda.Event()
            done.record(cur_stream)
            side.wait_event(done)
            L.check(L.lib().sos_conv2d_wgrad_reduce(ctypes.byref(d), ctypes.c_void_p(side.cuda_stream)), "sos_conv2d_wgrad_reduce")
            red = torch.cuda.Event()
            red.record(side)
            slot[1] = red
            _wg.pending[side.cuda_stream] = red
            WG_STATS["deferred"] += 1
            dw.record_stream(side)
        else:
            L.check(L.lib().sos_conv2d_wgrad(ctypes.byref(d), L.stream_ptr()), "sos_conv2d_wgrad")
            if end is not None:
                end.record()
        first = False
