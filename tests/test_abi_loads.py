"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/sos_hip.h declares; the module mirrors expose the reference's state_dict layout."""
import os
import re

import pytest
import torch

from oracle import nets as onet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("precision,storage", [("bf16", b"bf16"), ("bf16x3", b"bf16"), ("fp16", b"fp16")])
def test_library_exports_every_declared_symbol(precision, storage):
    """Both builds of the C ABI (libsos_hip.so: bfloat16 storage, libsos_hip_f16.so: IEEE half) export every symbol the
    header declares, and the ctypes table binds exactly those."""
    import sos_amd
    from sos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    declared = set(re.findall(r"\b(sos_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("sos_stream_t")
    assert declared, "header parse failed"
    sos_amd.set_precision(precision)
    try:
        h = _lib.lib()
    finally:
        sos_amd.set_precision("bf16")
    for name in declared:
        assert hasattr(h, name), f"{name} declared in sos_hip.h but not exported"
    assert set(_lib.SIGNATURES) | {"sos_last_error"} == declared
    assert h.sos_abi_version() == _lib.EXPECTED_ABI == 10
    assert h.sos_storage_dtype() == storage


def test_tune_table_load_rejects_foreign_and_illegal_entries(tmp_path):
    """sos_conv2d_tune_load (host only, no GPU): a table of another format / ABI is an error, an entry whose tiling the
    build would not offer for that shape is dropped, a legal one is accepted; the shipped table loads completely."""
    from sos_amd import _lib, engine
    h = _lib.lib()
    bad = tmp_path / "old.txt"
    bad.write_text("64 256 178 178 96 1 96 5 5 1 1 1 256 178 0 1 0 0 96 1 4 4 6\n")      # round-1 format: no header
    assert h.sos_conv2d_tune_load(str(bad).encode()) < 0
    shape = "64 256 178 178 96 1 96 5 5 1 1 1 256 178 0 1 0 0 96"
    mixed = tmp_path / "mixed.txt"
    mixed.write_text("sos_conv_tune 2 abi 3 nkey 19\n"
                     f"{shape} 1 4 4 6\n"            # legal: 16x16 pixels, 6 k-steps per chunk
                     f"{shape} 1 4 4 7\n"            # 7 does not divide cin/16
                     f"{shape} 4 2 4 6\n"            # 4 residue classes need dil_w >= 4
                     f"{shape} 1 8 8 6\n")           # 2^16 pixels per workgroup
    assert h.sos_conv2d_tune_load(str(mixed).encode()) == 1
    assert h.sos_conv2d_tune_load(str(tmp_path / "missing.txt").encode()) == 0
    if os.path.exists(engine.SHIPPED_TUNE_TABLE):
        lines = [ln for ln in open(engine.SHIPPED_TUNE_TABLE).read().splitlines()[1:] if ln.strip()]
        assert h.sos_conv2d_tune_load(engine.SHIPPED_TUNE_TABLE.encode()) == len(lines) > 0


def test_tile_count_refuses_fused_input_batchnorm_where_no_kernel_applies_it():
    """sos_conv2d_tile_count (host only, no launch) resolves a descriptor's tiling exactly as sos_conv2d_fwd does.  A fused input
    BatchNorm (sos_conv_desc.in_scale) on 48 -> 48 has no tiling whose kernel applies it (the 16-row kernel never reads in_scale,
    the fused instances are three n-tiles wide): the descriptor is refused with the reason, not given a tile count for a launch
    that would skip the BatchNorm."""
    import ctypes as C
    from sos_amd import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    d = L.ConvDesc()
    d.in_, d.wgt, d.out = p, p, p
    d.B, d.H, d.W, d.Wl = 2, 20, 20, 20
    d.in_cs, d.cin, d.in_nseg, d.in_seg_stride = 48, 48, 1, 48
    d.kh, d.kw, d.cout, d.cout_pad, d.cout_store = 5, 5, 48, 64, 48
    d.stride, d.dil_h, d.dil_w, d.pad_top, d.pad_left = 1, 1, 1, 2, 2
    d.Ho, d.Wo = 20, 20
    d.out_dtype, d.out_sc, d.out_sw, d.out_sh, d.out_sb = L.DT_BF16, 1, 48, 20 * 48, 400 * 48
    assert h.sos_conv2d_tile_count(C.byref(d)) > 0
    d.in_scale, d.in_shift = p, p
    assert h.sos_conv2d_tile_count(C.byref(d)) < 0
    assert "fused input BatchNorm" in h.sos_last_error().decode()


def test_wgrad_table_load_rejects_foreign_and_illegal_entries(tmp_path):
    """sos_wgrad_tune_load (host only, no GPU; ABI 7): a table of another format is an error, a plan the build would not offer
    for that shape is dropped, a legal one is accepted; the shipped table of measured weight-gradient plans loads completely."""
    from sos_amd import _lib, engine
    h = _lib.lib()
    bad = tmp_path / "foreign.txt"
    bad.write_text("sos_wgrad_tune 9 nkey 12\n")
    assert h.sos_wgrad_tune_load(str(bad).encode()) < 0
    shape = "256 178 5 5 1 4 4 96 96 0 0 0"          # Hg Wg kh kw stride dil_h dil_w M N 16x16x32-kernel temporal flat
    mixed = tmp_path / "mixed.txt"
    mixed.write_text("sos_wgrad_tune 1 nkey 12\n"
                     f"{shape} 3 1 0 4 1 1\n"        # legal: 3 m-tiles x 1 n-tile, 16 x 16 pixels, column-major, one workgroup per CU
                     f"{shape} 3 2 0 4 1 1\n"        # 2 n-tiles x 25 taps > 32 (tap, n-tile) pairs
                     f"{shape} 3 1 3 4 1 1\n"        # 8 residue classes need dil_w % 8 == 0
                     f"{shape} 4 1 0 4 1 1\n"        # 4 m-tiles
                     f"{shape} 3 1 0 4 1 2\n"        # two workgroups per CU: 3 m-tiles + the 5x5 patch do not fit half the LDS
                     "256 178 5 5 1 1 1 48 48 0 0 0 2 1 0 4 0 1\n")   # 48 x 48 x 25 taps is the 16x16x32 kernel's shape: flag mismatch
    assert h.sos_wgrad_tune_load(str(mixed).encode()) == 1
    assert h.sos_wgrad_tune_load(str(tmp_path / "missing.txt").encode()) == 0
    lines = [ln for ln in open(engine.SHIPPED_WGRAD_TABLE).read().splitlines()[1:] if ln.strip()]
    assert h.sos_wgrad_tune_load(engine.SHIPPED_WGRAD_TABLE.encode()) == len(lines)


def test_wgrad_table_load_asks_the_plan_legality_function_for_every_bound(tmp_path):
    """sos_wgrad_tune_load has no bounds of its own: an entry loads if and only if the one legality function (wg_make_plan) offers
    that plan, so it admits what SOS_WGRAD_OCC admits -- up to four workgroups per CU where the buffers fit a quarter of the
    LDS -- and nothing beyond."""
    from sos_amd import _lib
    h = _lib.lib()
    flat = "1 2900000 1 1 1 1 1 24 96 0 0 1"        # a flattened 1x1 gradient, 24 x 96 channels: one m-tile, up to three n-tiles
    t = tmp_path / "occ.txt"
    t.write_text("sos_wgrad_tune 1 nkey 12\n"
                 f"{flat} 1 1 0 0 0 3\n"             # three workgroups per CU: 16 KB + 16 KB + tables fit a third of the LDS
                 f"{flat} 1 1 0 0 0 5\n"             # five: more than any caller can ask for
                 f"{flat} 1 1 0 0 0 0\n"             # none
                 f"{flat} 1 4 0 0 0 1\n"             # four n-tiles of a 96-channel side
                 f"{flat} 2 1 0 0 0 1\n"             # two m-tiles of a 24-channel side
                 f"{flat} 1 1 0 0 2 1\n"             # a third pixel order
                 f"{flat} 1 1 7 0 0 1\n"             # 128 residue classes
                 f"{flat} 1 1 0 -1 0 1\n")           # half a row
    assert h.sos_wgrad_tune_load(str(t).encode()) == 1


def _wgrad_tune_desc():
    """A valid 3x3 descriptor over dummy (never dereferenced) pointers."""
    import ctypes as C
    from sos_amd import _lib as L
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    d = L.WgradDesc()
    d.g, d.x, d.partial, d.dw = p, p, p, p
    d.B, d.Hg, d.Wg, d.g_cs, d.Hx, d.Wx, d.x_cs = 2, 20, 20, 64, 20, 20, 96
    d.M, d.N, d.kh, d.kw, d.stride, d.dil_h, d.dil_w = 64, 96, 3, 3, 1, 1, 1
    d.pad_top, d.pad_left, d.scale = 1, 1, 1.0
    return d, buf


@pytest.mark.parametrize("field,value,message", [
    ("kw", 0, "bad descriptor"), ("M", 0, "bad descriptor"), ("stride+dil", 2, "bad descriptor"),
    ("temporal", 3, "bad temporal taps"), ("dw", None, "null pointer"), ("kw", 33, "taps per row not supported")],
    ids=["kw0", "M0", "stride2-dil2", "temporal", "null-dw", "33-taps-per-row"])
def test_wgrad_tune_validates_like_the_launch(field, value, message):
    """sos_wgrad_tune routes a descriptor exactly as sos_conv2d_wgrad does, so what the launch refuses the tuner refuses with the
    same code and message -- before any plan arithmetic (kw = 0 and M = 0 used to reach integer divisions by zero) and without
    touching the device (host only: the pointers are dummies, no GPU is needed)."""
    import ctypes as C
    from sos_amd import _lib as L
    h = L.lib()
    d, keep = _wgrad_tune_desc()
    if field == "stride+dil":
        d.stride, d.dil_h = value, value
    elif field == "temporal":
        d.t_taps, d.t_frames, d.t_cin = value, 2, 128          # N = 96 is not 3 x 128
    else:
        setattr(d, field, value)
    best = C.c_float(7.0)
    rc_tune = h.sos_wgrad_tune(C.byref(d), 1, C.byref(best), None)
    msg_tune = h.sos_last_error().decode()
    rc_launch = h.sos_conv2d_wgrad(C.byref(d), None)
    msg_launch = h.sos_last_error().decode()
    assert rc_tune == rc_launch and rc_tune < 0, (rc_tune, rc_launch)
    assert rc_tune == (-28 if field == "kw" and value == 33 else -22)          # SOS_ENOSPC / SOS_EINVAL
    assert message in msg_tune and message in msg_launch, (msg_tune, msg_launch)
    assert msg_tune.startswith("sos_wgrad_tune:" if field == "dw" else "sos_conv2d_wgrad:")
    assert best.value == 7.0                                    # refused: nothing was measured, nothing written


# lengths list -> (sdr filter_length 0, 512; stoi (p, q) = (1, 1), (5, 8); metric batch at 8 kHz (240, 60, 512), at 16 kHz (480, 120, 1024))
RAGGED_WORKSPACE_BYTES = {
    "one_sample": (1024, 8704, 256, 768, 1280, 1280),
    "one_chunk": (1024, 8704, 8448, 25856, 33536, 33536),
    "three": (2048, 353024, 333056, 1029120, 1315584, 1315584),
    "mixed_300": (212736, 48859648, 48235008, 149080832, 190613760, 190613760),
}


def test_ragged_workspace_sizes_are_the_recorded_ones():
    """sos_sdr_workspace_bytes, sos_stoi_workspace_bytes and sos_metric_batch_workspace_bytes (host only) lay their arrays out
    with one shared helper (csrc/ragged.h).  The expected byte counts are literals: the same calls were made against the library
    of the commit before the shared header, on a CPU, and every offset and total was to stay that number."""
    import ctypes as C
    import numpy as np
    from sos_amd import _lib
    h = _lib.lib()
    lists = {"one_sample": [1], "one_chunk": [4096], "three": [4097, 1, 160000],
             "mixed_300": [int(v) for v in np.random.default_rng(11).integers(1, 160001, size=300)]}
    assert set(lists) == set(RAGGED_WORKSPACE_BYTES)
    for name, ls in lists.items():
        a = np.asarray(ls, dtype=np.int64)
        p, n = a.ctypes.data_as(C.c_void_p), len(a)
        got = (h.sos_sdr_workspace_bytes(p, n, 0), h.sos_sdr_workspace_bytes(p, n, 512),
               h.sos_stoi_workspace_bytes(p, n, 1, 1), h.sos_stoi_workspace_bytes(p, n, 5, 8),
               h.sos_metric_batch_workspace_bytes(p, n, 240, 60, 512), h.sos_metric_batch_workspace_bytes(p, n, 480, 120, 1024))
        assert got == RAGGED_WORKSPACE_BYTES[name], (name, got)
    for bad_p, bad_n in ((p, 0), (p, 65536), (None, 3)):
        assert h.sos_sdr_workspace_bytes(bad_p, bad_n, 512) == -1
        assert h.sos_stoi_workspace_bytes(bad_p, bad_n, 5, 8) == -1
        assert h.sos_metric_batch_workspace_bytes(bad_p, bad_n, 480, 120, 1024) == -1


def test_state_dict_keys_match_reference_layout():
    from sos_amd.detector import networks as dnet
    from sos_amd.denoiser import networks as jnet
    from sos_amd.common import MyConfig
    det = dnet.get_network()
    spec = onet.detector_spec()
    sd = det.state_dict()
    assert list(sd.keys()) == [k for k, _, _ in spec]
    assert all(tuple(sd[k].shape) == tuple(s) for k, s, _ in spec)
    jm = jnet.get_network(MyConfig())
    spec = onet.joint_spec()
    sd = jm.state_dict()
    assert list(sd.keys()) == [k for k, _, _ in spec]
    assert all(tuple(sd[k].shape) == tuple(s) for k, s, _ in spec)
    # strict load of a reference-shaped checkpoint works
    jm.load_state_dict(onet.closed_form_state(spec, seed=2), strict=True)


def test_no_cpu_fallback():
    from sos_amd.detector import networks as dnet
    from sos_amd import transform
    det = dnet.get_network().eval()
    with pytest.raises(RuntimeError):
        det(torch.zeros(1, 2, 256, 64))
    with pytest.raises(RuntimeError):
        transform.stft_batch(torch.zeros(1, 28000))


def test_lstm_gate_permutation_is_consistent():
    """engine.lstm_gate_perm: torch's (dir, gate, unit) row order -> the kernels' gate-interleaved (dir, unit, gate)
    order (include/sos_hip.h: channel dir*4H + 4*j + q), and its inverse."""
    import torch
    from sos_amd import engine as E
    H = 12
    perm, inv = E.lstm_gate_perm(H, torch.device("cpu"))
    assert sorted(perm.tolist()) == list(range(8 * H))
    assert torch.equal(perm[inv], torch.arange(8 * H)) and torch.equal(inv[perm], torch.arange(8 * H))
    for d in range(2):
        for j in range(H):
            for q in range(4):
                assert int(perm[d * 4 * H + 4 * j + q]) == d * 4 * H + q * H + j


def test_bench_picks_the_dominant_signature_by_work_not_by_warm_up_time():
    """bench.py's roofline leg: the dominant launch signature is the one carrying the most algorithmic FLOPs (per launch x
    launches), whatever one-time host work inflated the HIP-event brackets of other signatures during warm-up (a run once
    reported a 15 TFLOP/s first-layer gradient as dominant: roofline.frac 0.005)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    summ = {("conv", 5, 5, 1, 1, 1, 96, 96, 64, 256, 178): dict(flops=1.344e12, launches=12, total_ms=14.0, avg_ms=1.17),
            ("conv", 5, 5, 2, 2, 1, 96, 96, 64, 256, 178): dict(flops=1.344e12, launches=6, total_ms=7.2, avg_ms=1.2),
            ("wgrad", 1, 7, 1, 1, 1, 48, 2, 64, 256, 178): dict(flops=3.9e9, launches=6, total_ms=900.0, avg_ms=150.0)}
    assert bench._dominant(summ) == ("conv", 5, 5, 1, 1, 1, 96, 96, 64, 256, 178)
