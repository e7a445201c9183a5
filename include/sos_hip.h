/* sos_hip.h -- C ABI of libsos_hip.so, the MI355X (gfx950) hot path of the
 * Listening-to-Sound-of-Silence speech-denoising pipeline.
 *
 * The reference is pure Python/PyTorch: it has no FFI or operator registry, so
 * the drop-in seam is its Python module API.  Each entry point
 * below is what the thin Python shims in
 * listening-to-sound-of-silence-for-speech-denoising_amd/ bind through ctypes;
 * the comment on each cites the reference function it replaces
 * (paths relative to /root/reference, M1 = model_1_silent_interval_detection/
 * audioonly_model, M2 = model_2_audio_denoising/audio_denoising_model).
 *
 * Conventions: every pointer is a DEVICE pointer unless said otherwise; no
 * allocation and no synchronisation inside; work is enqueued on `stream`
 * (a hipStream_t); return 0 on success, negative on error (message via
 * sos_last_error()).  No C++ exceptions cross this boundary.
 */
#ifndef SOS_HIP_H
#define SOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sos_stream_t; /* hipStream_t */

enum { SOS_OK = 0, SOS_EINVAL = -22, SOS_ELAUNCH = -5, SOS_ENOSPC = -28 };

/* activation / padding / dtype codes */
enum { SOS_ACT_NONE = 0, SOS_ACT_RELU = 1, SOS_ACT_PRELU = 2, SOS_ACT_SIGMOID = 3 };
enum { SOS_PAD_ZERO = 0, SOS_PAD_REFLECT = 1 };
enum { SOS_DT_BF16 = 0, SOS_DT_BF16X3 = 1, SOS_DT_F32 = 2 };

int sos_abi_version(void);
/* size in bytes of the descriptor structs as compiled into the library; which = 0: sos_view, 1: sos_conv_desc,
 * 2: sos_wgrad_desc; anything else: -1 */
int sos_struct_size(int which);
const char* sos_last_error(void);
/* The package builds this ABI twice from the same sources: libsos_hip.so computes on bfloat16 storage ("bf16"),
 * libsos_hip_f16.so on IEEE half ("fp16", same MFMA rate, 11 instead of 8 significand bits).  Wherever this header
 * says "bf16" for an activation / packed-weight buffer it means "the library's 16-bit storage type". */
const char* sos_storage_dtype(void);

/* Front-end geometry (a1, a2): librosa 0.7.1 stft / istft semantics (hann-periodic window of win_length centred in n_fft,
 * center=True, reflect padding, length=None) for even 16 <= n_fft <= 2048, 16 <= win_length <= n_fft,
 * 1 <= hop <= n_fft (odd hops included) and ceil(win_length/hop) <= 16; clips need n_samples > n_fft/2.  Any other
 * geometry is SOS_EINVAL from every a1 / a2 entry point (the *_matrix_bytes functions return -1) and sos_last_error()
 * names the rule violated.
 *
 * ---- a1  fast_stft: M1/transform.py:188-193 (librosa.stft(data,510,158,400), hann-periodic window centred in
 * n_fft, center=True, reflect pad) fused with real_imag_expand (:10-17) and the caller's transpose to [2,F,T]
 * (M2/dataset.py:255).  The transform is a windowed-DFT GEMM on the matrix cores (csrc/stft_mfma.hip): the constant
 * matrix is packed ONCE on the host into MFMA fragment order, as hi + lo half-precision parts (the product is taken as
 * hi*hi + hi*lo + lo*hi with fp32 accumulation, ~22 significand bits), and uploaded by the caller:
 *   sos_stft_matrix_bytes(): bytes of ONE part; sos_stft_pack_matrix(): fills two HOST buffers of that size.
 * wave f32 [B][wave_stride], out f32 [B][2][n_fft/2+1][T], T = 1 + n_samples/hop.  Geometry: see above; the packed
 * matrix is zero-padded to ceil(2*(n_fft/2+1)/32) row tiles and ceil(win_length/16) k-steps. */
int64_t sos_stft_matrix_bytes(int n_fft, int hop, int win_length);
int sos_stft_pack_matrix(int n_fft, int hop, int win_length, void* hi /* host */, void* lo /* host */);
int sos_stft_f32(const float* wave, int64_t batch, int64_t n_samples, int64_t wave_stride,
                 const void* mat_hi, const void* mat_lo /* device copies of the packed matrix */, int n_fft, int hop,
                 int win_length, float* out, int64_t n_frames,
                 const int32_t* clip_samples /* optional device [B], ragged batch: clip b has clip_samples[b] <= n_samples
                    samples (reflected at ITS end) and 1 + clip_samples[b]/hop frames; rows keep the pitch n_frames */,
                 sos_stream_t stream);

/* ---- a2  fast_istft: M1/transform.py:196-202 (librosa.istft(S,158,400)): inverse real DFT, synthesis window,
 * overlap-add, division by the window-sum-square (where > tiny), trim n_fft/2 both ends -- the synthesis GEMM
 * (window and irfft weights folded into the packed matrix, same hi/lo scheme), then a fixed-order overlap-add of the
 * <= ceil(win/hop) frames covering a sample with the window-sum-square taken over those same frames; samples whose
 * window-sum-square is <= FLT_MIN (gaps when hop > win) are not divided.  Geometry: see above; the packed matrix is
 * zero-padded to ceil(win_length/32) row tiles and K = 2*(n_fft/2+1) rounded up to a multiple of 64.
 * sos_istft_pack_matrix also fills win_sq f32 [win_length] (HOST), the squared window.
 * spec f32 [B][2][F][T]; out f32 [B][out_stride], hop*(T-1) samples written. */
int64_t sos_istft_matrix_bytes(int n_fft, int hop, int win_length);
int sos_istft_pack_matrix(int n_fft, int hop, int win_length, void* hi /* host */, void* lo /* host */, float* win_sq /* host */);
int sos_istft_f32(const float* spec, int64_t batch, int64_t n_frames, const void* mat_hi, const void* mat_lo,
                  const float* win_sq /* device */, int n_fft, int hop, int win_length, float* out, int64_t out_stride,
                  const int32_t* clip_frames /* optional device [B], ragged batch: clip b has clip_frames[b] <= n_frames
                     frames -> hop*(clip_frames[b]-1) samples */,
                  sos_stream_t stream);

/* power_law: M1/transform.py:178-185, out = sign(x) |x|^power -- the optional companding of fast_stft / fast_istft
 * (`power=True`: 0.3 before the STFT, 1/0.3 after the ISTFT). */
int sos_power_law_f32(const float* x, int64_t n, float power, float* out, sos_stream_t stream);

/* ---- a4/a5  batch_fast_icRM_sigmoid: M1/transform.py:156-169 (and the numpy
 * twin fast_icRM_sigmoid :141-153): M = (1/a)(log(c/(1-c+1e-8)+1e-10)+b), rec = M*Y
 * (complex).  Y, crm, rec: f32 [B][2][plane]. */
int sos_crm_apply_f32(const float* Y, const float* crm, float* rec, int64_t batch, int64_t plane,
                      float a, float b, sos_stream_t stream);
/* backward of the above w.r.t. crm (grad flows to the mask, M2/agent.py:186-189). */
int sos_crm_apply_bwd_f32(const float* Y, const float* crm, const float* grad_rec, float* grad_crm,
                          int64_t batch, int64_t plane, float a, sos_stream_t stream);
/* ---- a3  fast_cRM_sigmoid: M1/transform.py:130-138 (generate_cRM :36-54 +
 * cRM_sigmoid_compress :92-94).  clean, mix, out: f32 [B][2][plane]. */
int sos_crm_target_f32(const float* clean, const float* mix, float* out, int64_t batch, int64_t plane,
                       float a, float b, sos_stream_t stream);

/* ---- a13/a15  convert_bitstreammask_to_audiomask: M2/tools.py:340-362 (=
 * M1/tools.py:770-792, M2/predict.py:232-252) + `noise_sig = mixed*mask`
 * (M2/predict.py:317).  bits u8 [B][n_frames] (1 = non-silent); mask f32
 * [B][n_samples] (1 on silent samples); if sig != NULL, masked = sig*mask.
 * Integer index rule evaluated in IEEE double exactly like the Python. */
int sos_bits_to_mask(const uint8_t* bits, int64_t batch, int64_t n_frames, double ratio,
                     int64_t n_samples, float* mask, const float* sig, float* masked,
                     const int32_t* clip_frames, const int32_t* clip_samples /* optional device [B] each, ragged batch:
                        clip b has clip_frames[b] bits and clip_samples[b] samples; row pitches stay n_frames / n_samples */,
                     sos_stream_t stream);

/* ---- a16  add_signals / add_noise_to_audio: M2/tools.py:217-303.  Per clip b: every noise k is rescaled so that
 * energy(signal) / energy(noise) = 10^(snr_db[b]/10) (left alone when signal or noise is silent), mixed = signal +
 * sum_k noise_k, then mixed, signal and the noises are divided by max|mixed| / norm (norm == 0: no normalisation).
 * signal f32 [B][n], noises f32 [B][n_noises][n] (n_noises <= 8), snr_db f32 [B] (device); outputs same shapes. */
int sos_add_signals_f32(const float* signal, const float* noises, const float* snr_db, int64_t batch, int n_noises,
                        int64_t n, float norm, float* mixed, float* signal_out, float* noises_out, sos_stream_t stream);

/* ---- a14  detector post-processing: M1/predict.py:117-119,
 * bit = sigmoid(logit) >= 0.5 (1 = non-silent).  conf (optional) = sigmoid. */
int sos_threshold_bits(const float* logits, int64_t n, float threshold, uint8_t* bits, float* conf,
                       sos_stream_t stream);
/* Two-pass detector of the 'mixed' pipeline (the threshold of M1/predict.py:117-119 only depends on the SIGN of a logit):
 * logits f32 [B][n] of a 1x-cost 16-bit detector pass; clip b is MARKED (mark[b] = 1) when one of its first n_valid[b] (NULL: n)
 * frames has |logit| < band_rel * max(1, max_t |logit[b][t]|, max_t scale[b][t]), i.e. lies inside the 16-bit pass's error band
 * around the threshold.  scale (ABI 10; optional f32 [B][n]): the magnitude that error is relative to -- the last layer's
 * sum_i |w_i| |a_i| + |bias| per frame (>= |logit|), so that logits that are small by cancellation do not shrink the band.  tabs_in / tabs_out int32 [ntab][B]: per-clip width tables of the ragged geometry (sos_conv_desc.wl_tab / wo_tab,
 * the BiLSTM's lengths, ...): tabs_out = tabs_in for marked clips, 0 for the others, so that a second detector pass in the
 * parity precision computes ONLY the marked clips (tiles of a zero-width clip exit at once) without a host round trip.
 * count (optional int32 [2]) += {marked clips, clips}. */
int sos_logit_band_mark(const float* logits, const float* scale, int64_t batch, int64_t n, const int32_t* n_valid,
                        float band_rel, const int32_t* tabs_in, int32_t* tabs_out, int ntab, int32_t* mark, int32_t* count,
                        sos_stream_t stream);

/* ---- layout glue at the module boundary: f32 NCHW [B][C][H][W] -> bf16 NHWC
 * [B][H][W][cs] (channels >= C zero filled; SOS_DT_BF16X3 writes hi|hi|lo thirds
 * of width cs/3). */
int sos_pack_nchw_to_nhwc(const float* in, int64_t B, int C, int64_t H, int64_t W, void* out, int cs,
                          int dtype, const float* mul /* optional device scalar multiplied in (loss scale) */,
                          sos_stream_t stream);
/* The same boundary pack with the kw HORIZONTAL TAPS of the first conv layer folded into the channel axis: stored channel
 * t*C + c of pixel (h, w) = in[b][c][h][w + t - pad_left] (t < kw; outside the clip: zero for SOS_PAD_ZERO, mirrored for
 * SOS_PAD_REFLECT; channels >= kw*C zero).  The first block of every encoder (Conv2d(2, nf, (1,7)), M1/networks.py:120-128,
 * M2/networks.py:72-80) and of the U-Net (DownConvBlock(2, 64, 5, 1), M2/networks.py:158,165) then runs as a kh x 1 layer over
 * kw*C real channels with the weight w'[o][t*C + c][a][0] = w[o][c][a][t] -- 14 or 10 of the 16 stored channels real instead
 * of 2, at no extra byte.  clip_w: optional device [B] (ragged batch: clip b has clip_w[b] <= W columns, its border is taken
 * at ITS end, columns past it are written as zeros).  cs (per third) % 8 == 0 and >= kw*C. */
int sos_pack_nchw_wtaps(const float* in, int64_t B, int C, int64_t H, int64_t W, int kw, int pad_left, int pad_mode,
                        const int32_t* clip_w, void* out, int cs, int dtype, const float* mul, sos_stream_t stream);

/* ---- a6,a8,a9 (+ a7/a10/a11 heads): Conv2d (zero or reflect pad, stride,
 * dilation) / ConvTranspose2d phases / Linear, fused with folded BatchNorm or bias
 * and ReLU / PReLU / Sigmoid -- M1/networks.py:28-51, M2/networks.py:28-51,97-149.
 * Implicit GEMM on bf16 MFMA, fp32 accumulate. */
typedef struct sos_conv_desc {
    /* input activation, bf16 NHWC: element (b,h,w,c) at ((b*H + h)*W + w)*in_cs + c */
    const void* in;
    int32_t B, H, W;        /* physical input dims                                     */
    int32_t in_cs;          /* channels stored per pixel (multiple of 8)               */
    int32_t cin_off, cin;   /* contracted channel range [cin_off, cin_off+cin), cin%16==0 */
    int32_t in_nseg;        /* number of such ranges (1, or 3 for the hi|hi|lo thirds)   */
    int32_t in_seg_stride;  /* channel distance between consecutive ranges               */
    const int32_t* w_gather;/* optional [Wl]: physical column of logical column (nearest resize) */
    int32_t Wl;             /* logical input width (== W when w_gather == NULL)        */
    /* weights, bf16 [kh*kw][cout_pad][in_nseg*cin], cout_pad % 32 == 0                */
    const void* wgt;
    int32_t kh, kw, cout, cout_pad;
    int32_t stride, dil_h, dil_w, pad_top, pad_left, pad_mode;
    /* output: pixel (b,ho,wo), channel co at out + b*sb + ho*sh + wo*sw + (c_off+co)*sc  */
    int32_t Ho, Wo;
    void* out;
    int32_t out_dtype;      /* SOS_DT_*                                                */
    int64_t out_sb, out_sh, out_sw, out_sc;
    int32_t out_c_off;
    int32_t cout_store;     /* channels [cout, cout_store) are written as zero          */
    int64_t out_third;      /* SOS_DT_BF16X3: element distance between hi|hi|lo thirds  */
    /* epilogue: y = act(acc*scale[co] + shift[co]); scale == shift == NULL: y = act(acc)  */
    const float* scale;     /* [cout_pad]                                               */
    const float* shift;     /* [cout_pad]                                               */
    int32_t act;            /* SOS_ACT_*                                                */
    const float* act_param; /* device scalar (PReLU slope) or NULL                      */
    int32_t accumulate;     /* 1: add to the existing bf16 output (dense NHWC outputs only): gradient
                               fan-in of skip connections in the backward pass            */
    /* optional fused BatchNorm statistics of the (bf16-rounded) output, dense bf16 NHWC outputs only:
     * stats[0][c][tile] = sum, stats[1][c][tile] = sum of squares over the tile's valid pixels, c < stats_c,
     * tile < sos_conv2d_tile_count(desc) (2 * stats_c * tiles floats; a channel's tile sums are contiguous for the
     * finalize); feed to sos_bn_finalize(partial = stats, nblk = tile count). */
    float* stats;
    int32_t stats_c;
    /* optional RAGGED batch (BASELINE configs[3]: clips of different lengths in one launch; the reference runs each
     * file at its own length, M2/predict.py:405-447): the buffers keep the geometry above with W / Wl / Wo = the
     * batch's maxima, image b uses only its first wl_tab[b] logical input columns (zero / reflect borders are taken
     * at ITS end) and produces wo_tab[b] output columns; the rest of its output columns are left untouched.  Device
     * int32 [B] each, both or neither.  w_gather_stride: distance in ints between the images' w_gather tables
     * (0: one table for all). */
    const int32_t* wl_tab;
    const int32_t* wo_tab;
    int32_t w_gather_stride;
    /* optional TEMPORAL taps (Conv3d with temporal stride 1 and padding (kt-1)/2, M1/networks.py:54-77: the audio-visual
     * variant's video branch): the B images are clips of t_frames consecutive frames and the contraction also runs over
     * t_taps neighbouring frames, image b reading frames b + dt - t_pad (dt < t_taps) of ITS clip, zeros outside the
     * clip.  The contraction index is (range s < in_nseg, dt, channel): weights [kh*kw][cout_pad][in_nseg*t_taps*cin].
     * t_taps <= 1: plain 2-D convolution.  Replaces a materialised time-stacked input (sos_time_stack). */
    int32_t t_frames, t_taps, t_pad;
    /* optional REFLECTION-PAD FOLD of the output (backward of ReflectionPad2d in DownConvBlock, M2/networks.py:105: the data
     * gradient of a reflect-padded conv is a full correlation onto the PADDED domain [H+2p][W+2p] whose border cells add to the
     * interior cell they mirror).  fold_pad = p > 0: output pixel (ho, wo) is cell (hp, wp) = (ho*fold_sy + fold_oy,
     * wo*fold_sx + fold_ox) of the padded domain (sy = sx = 1, oy = ox = 0 for a stride-1 layer; 2 and the phase for the four
     * phase convolutions of a stride-2 layer).  Interior cells (p <= hp < p + fold_H, p <= wp < p + fold_W) are written -- with
     * `accumulate`: added -- straight to `out` as pixel (hp - p, wp - p) of the dense [B][fold_H][fold_W] NHWC tensor that
     * out_sb / out_sw / out_c_off / out_third describe (out_sh is ignored); border cells are stored to the padded scratch tensor
     * fold_pad_out, dense [B][fold_H+2p][fold_W+2p][fold_row] with the channels from 0 (thirds fold_third apart), which
     * sos_reflect_fold_border then adds onto `out`.  Only the border of the scratch tensor is ever touched.  16-bit NHWC outputs
     * (out_sc == 1) without fused statistics only. */
    void* fold_pad_out;
    int32_t fold_pad, fold_H, fold_W, fold_sy, fold_oy, fold_sx, fold_ox, fold_row;
    int64_t fold_third;
    /* optional FUSED INPUT BatchNorm + ReLU (round 5; Conv2dBlock, M2/networks.py:28-51, training mode): `in` holds the RAW conv
     * output of the producing block and in_scale / in_shift (f32 [cin], channel c of the contraction = input channel cin_off + c)
     * its batch-statistics scale / shift: every value read becomes max(x * in_scale[c] + in_shift[c], 0), rounded to the storage
     * type exactly as sos_bn_act_apply would have stored it, while the patch is staged; zero padding stays zero.  The separate
     * apply pass and the activated tensor are then not needed by this consumer.  One 16-bit channel segment, no temporal taps;
     * built for the 96-channel context layers' tilings -- three n-tiles, 2 or 3 k-steps, patches of at most 64 staging instructions
     * (768 / 576 pixels): other tilings are not offered to such a descriptor (EINVAL if none is left: the caller falls back to the
     * materialised tensor). */
    const float* in_scale;
    const float* in_shift;
} sos_conv_desc;

int sos_conv2d_fwd(const sos_conv_desc* desc /* host pointer */, sos_stream_t stream);
/* number of pixel tiles (workgroup columns) the NEXT sos_conv2d_fwd of this shape will use: the tuned tiling if
 * sos_conv2d_tune has run for the shape, the default otherwise */
int64_t sos_conv2d_tile_count(const sos_conv_desc* desc);

/* One-time autotune for the SHAPE of `desc` (not its pointers): runs the `max_candidates` most
 * promising tilings `iters` times each, timed with HIP events on `stream` (this call
 * SYNCHRONISES -- keep it out of graph capture and timed regions), and caches the winner for
 * every later sos_conv2d_fwd of the same shape.  *best_ms (optional) = winning time, or -1 if
 * the shape was already tuned. */
int sos_conv2d_tune(const sos_conv_desc* desc, int max_candidates, int iters, float* best_ms,
                    sos_stream_t stream);
/* Save / load the tuned-tiling cache (host text file).  load returns the number of entries read. */
int sos_conv2d_tune_save(const char* path);
int sos_conv2d_tune_load(const char* path);

/* ---- a7/a11 recurrent part of nn.LSTM(bidirectional=True), gate order i,f,g,o
 * (M1/networks.py:95,143-148; M2/networks.py:64,88).  The input projection
 * x@W_ih^T + b_ih + b_hh is a sos_conv2d_fwd (1x1) producing xproj.
 * W_hh (f32 [2][4H][H], the layout torch stores: weight_hh_l0, weight_hh_l0_reverse) is packed once per
 * weight version into MFMA fragment order: sos_lstm_pack_bytes(H, 0 / 1) = bytes of ONE forward /
 * backward array; the lo arrays (both or neither) hold the bf16 remainders for the three-pass
 * hi*hi + hi*lo + lo*hi product of the bf16x3 precision mode.  H % 4 == 0, H <= 256.
 * xproj f32 [B][T][2][4H] (dir 0 fwd, 1 reverse) in GATE-INTERLEAVED order: channel dir*4H + 4*j + q for
 * hidden unit j and gate q in i,f,g,o (permute the rows of W_ih and of the bias; torch's order is q*H + j);
 * out_bf16 bf16 [B][T][out_cs] (+ thirds when dtype == SOS_DT_BF16X3). */
int64_t sos_lstm_pack_bytes(int H, int backward);
int sos_lstm_pack_whh(const float* whh, int H, void* fwd_hi, void* fwd_lo, void* bwd_hi, void* bwd_lo,
                      sos_stream_t stream);
int sos_lstm_bidir_fwd(const float* xproj, const void* wpk_hi, const void* wpk_lo /* optional */, int64_t B, int64_t T,
                       int H, void* out_bf16, int out_cs, int out_dtype, int64_t out_third,
                       float* save_gates /* optional f32, ceil16(B)*T*2*4H: post-activation i,f,g,o */,
                       float* save_c /* optional f32, ceil16(B)*T*2*H: cell state */,
                       const int32_t* lengths /* optional device [B]: clip b has lengths[b] <= T frames (ragged batch:
                          its reverse pass starts at frame lengths[b]-1; rows past it are neither read nor written) */,
                       sos_stream_t stream);
/* save_gates / save_c are consumed only by sos_lstm_bidir_bwd; their layout is the forward kernel's MFMA lane order
 * [16-clip group][t][dir][4-unit tile][clip][unit][i,f,g,o] (one coalesced store per tile and step). */

/* ---------------------------------------------------------------- training-mode kernels
 * A `sos_view` describes a channel slice of a bf16 NHWC activation: element (pix, c) lives at
 * ptr[pix*row + c_off + c]; with x3 != 0 the value is hi + lo, hi at that address (and again at
 * +third), lo at +2*third.  1 <= C <= 2048; row, c_off (and third) are multiples of 8.
 *
 * The 8-channel run.  The kernels that take views move 16-byte runs of 8 channels and do NOT mask by C: a view covers
 * the channels [c_off, c_off + pad8(C)), pad8(C) = C rounded up to a multiple of 8.  The slice must lie inside the row
 * (inside the third with x3 != 0): c_off + C <= row resp. third, which the library does not check; the rounded-up run
 * then lies inside it too, because row, third and c_off are multiples of 8.  With C % 8 != 0 the caller owns the padding
 * channels [c_off + C, c_off + pad8(C)) of every view it passes:
 *   - sos_copy_crop writes there what the source view holds in ITS padding channels (zero outside the overlap);
 *   - sos_reflect_fold / sos_reflect_fold_border fold the padded view's padding channels like real ones and store (or,
 *     accumulating, add) the result there: zero padding in `padded` keeps an accumulated destination's values (re-stored,
 *     in the three-pass mode possibly as another hi/lo pair of the same sum), a storing fold zeroes them;
 *   - sos_act_bwd_from_y and sos_feat_to_nhwc (C <= 8 in one aligned run) write zeros there.
 * These kernels touch no channel below c_off or at or beyond c_off + pad8(C).  sos_pack_grad_f32 writes exactly C channels
 * (its 8-channel row path needs C % 8 == 0).  The video glue of csrc/video.hip takes plain pointers and channel counts:
 * sos_time_stack, sos_time_unstack and sos_spatial_mean_bwd write whole rows with the padding channels zero,
 * sos_spatial_mean exactly C channels of the feature row.  The package's calls of the crop and the folds pass
 * C % 8 == 0 everywhere but one: the pad = 0 fold that adds the 2-channel loss gradient (a pack whose channels >= 2 are
 * zero) onto a 16-wide gradient buffer. */
typedef struct sos_view {
    void* ptr;
    int64_t npix;
    int32_t row, c_off, C, x3;
    int64_t third;
} sos_view;

/* ---- BatchNorm2d(train) of Conv2dBlock/ConvBlock/DownConvBlock/UpConvBlock (M1/networks.py:38-39,
 * M2/networks.py:38-39,107-108,137-138): batch statistics over all pixels of the raw conv output.
 * Stage 1 writes deterministic per-workgroup partial sums (no atomics): partial f32 [2][C][nblk] (a channel's sums contiguous),
 * nblk = sos_bn_stats_blocks(npix). */
int sos_bn_stats_blocks(int64_t npix);
int sos_bn_stats(const sos_view* x, float* partial, sos_stream_t stream);
/* Stage 2: mean / biased var -> scale = gamma*invstd, shift = beta - mean*scale (for the apply
 * pass), save_mean / save_invstd (for backward); running stats updated with momentum and the
 * UNBIASED variance, num_batches_tracked += 1 (torch semantics).  gamma/beta may be NULL (=1/0). */
int sos_bn_finalize(const float* partial, int nblk, int C, int64_t count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* scale, float* shift, float* save_mean, float* save_invstd, sos_stream_t stream);
/* y = act(x*scale + shift).  Dense form: y is a sos_view with the same npix.  Feature form
 * (feat_H > 0): the reference's view(B,-1,T).permute(2,0,1) (+ optional nearest-resize column
 * gather): pixel (b,h,w'), channel c is written to y.ptr[(b*feat_Wo + w')*y.row + (y.c_off + c)*feat_H + h]
 * reading source column w = gather ? gather[w'] : w' of a [B][feat_H][feat_W] pixel grid. */
int sos_bn_act_apply(const sos_view* x, const float* scale, const float* shift, int act, const float* slope,
                     const sos_view* y, int feat_H, int feat_W, int feat_Wo, const int32_t* gather,
                     sos_stream_t stream);

/* ---- weight gradient of Conv2d / ConvTranspose2d / Linear (autograd of F.conv2d etc. behind
 * loss.backward(), M1/agent.py:106-111, M2/agent.py:101-106):
 *   dw[m][n][a][b] (+)= scale * sum_p G[p][m] * X[p*stride + (a,b)*dil - pad][n]
 * G ("tile side"): bf16 NHWC [B][Hg][Wg][g_cs], channels [g_off, g_off+M); X ("patch side"): bf16
 * NHWC [B][Hx][Wx][x_cs], channels [x_off, x_off+N).  Conv: G = grad of the raw conv output,
 * X = layer input.  ConvTranspose2d(k3,s2,p1): G = layer input, X = output grad, stride 2 ->
 * result is in the (Cin, Cout, kh, kw) layout.  partial: fp32 workspace of
 * sos_wgrad_workspace_bytes(); dw fp32 [M][N][kh][kw]. */
typedef struct sos_wgrad_desc {
    const void* g;
    int32_t B, Hg, Wg, g_cs, g_off;
    const void* x;
    int32_t Hx, Wx, x_cs, x_off;
    int32_t M, N, kh, kw, stride, dil_h, dil_w, pad_top, pad_left, pad_mode;
    int32_t ksplit;         /* pixel-range split (parallelism), <= 0: automatic (one workgroup per CU); partial
                             * sums are reduced deterministically.  Size `partial` with sos_wgrad_workspace_bytes */
    float* partial;
    float* dw;
    int32_t accumulate;     /* 0: dw = result, 1: dw += result */
    float scale;
    const float* scale_dev; /* optional device scalar multiplied into `scale` (1 / loss scale of the fp16 mode) */
    /* optional TEMPORAL taps (see sos_conv_desc): N = t_taps * t_cin columns, column n = dt * t_cin + c pairs image b of
     * G with channel c of frame b + dt - t_pad of X (same clip of t_frames frames, zeros outside); t_cin % 128 == 0.
     * t_taps <= 1: off. */
    int32_t t_frames, t_taps, t_pad, t_cin;
} sos_wgrad_desc;
int64_t sos_wgrad_workspace_bytes(const sos_wgrad_desc* desc);
int sos_conv2d_wgrad(const sos_wgrad_desc* desc, sos_stream_t stream);
/* ABI 8: the two halves of sos_conv2d_wgrad as separate entry points -- _partial launches the MFMA kernel (per-split partial sums
 * into desc->partial), _reduce the deterministic reduction of those sums into desc->dw (scale, scale_dev, accumulate).  Both derive
 * the same launch plan from the descriptor, so the reduce may run on ANOTHER stream behind an event (the gradient is needed only by
 * the optimizer; engine.wgrad(defer=True) keeps a ring of workspaces and joins before the gradients are used). */
int sos_conv2d_wgrad_partial(const sos_wgrad_desc* desc, sos_stream_t stream);
int sos_conv2d_wgrad_reduce(const sos_wgrad_desc* desc, sos_stream_t stream);
/* ABI 7: measured launch plans of sos_conv2d_wgrad (workgroup channel tile, pixel tile, pixel order, workgroups per CU), the
 * counterpart of sos_conv2d_tune: times the candidate plans for the SHAPE of `desc` (`iters` launches each, the fastest few
 * again over 8x as many; HIP events on `stream`, SYNCHRONISES, overwrites desc->dw / desc->partial: pass accumulate = 0 and
 * scratch outputs) and caches the winner for every later sos_conv2d_wgrad of that shape.  *best_ms (optional) = the winning time,
 * -1 if the shape already had a plan (or takes the GEMM or a streaming path, which have none).  A descriptor sos_conv2d_wgrad
 * refuses is refused here with the same code and message, before anything is launched.  save / load: host text file; load returns the entries accepted
 * (0: no file).  The package ships wgrad_table_gfx950.txt so that every process and rank runs the same plans. */
int sos_wgrad_tune(const sos_wgrad_desc* desc, int iters, float* best_ms, sos_stream_t stream);
int sos_wgrad_tune_save(const char* path);
int sos_wgrad_tune_load(const char* path);
/* Host-only query of the launch sos_conv2d_wgrad would make for `desc` right now (run-time knobs, measured table and cached plans
 * as they stand): launches nothing, needs no GPU and dereferences no pointer of the descriptor (they only have to be non-null).
 * Returns the code the launch would return (SOS_EINVAL / SOS_ENOSPC for a refused descriptor, message in sos_last_error) and, on
 * SOS_OK, fills the first min(n_out, SOS_WGRAD_DESCRIBE_N) ints of `out`:
 *    0 route: 0 split-K GEMM, 1 thin 1x1 streaming kernel, 2 thin kh x 1 (taps) streaming kernel, 3 tiled kernels
 *    1 kernel kind: 0 wgrad_kernel<MT, NTB, BAL>, 1 wgrad16_kernel<M16, N16, FT>, 2 wgrad_thin_kernel<M16, N16>,
 *                   3 wgrad_thin_taps_kernel<M16, KH>, 4 wgrad_gemm_kernel
 *    2..4 the template arguments a, b, v of the kernel instance that resolved (0 where the kind has fewer)
 *    5 ksplit (partial planes the reduce folds), 6 grid size (workgroups), 7 dynamic LDS bytes
 *    tiled route only (0 elsewhere):
 *    8 MT, 9 NTB, 10 NC (residue classes), 11 log2 TH, 12 log2 TW, 13 pixel order, 14 workgroups per CU of the plan,
 *    15 dbuf (two operand buffers), 16 xcdmap (XCD-aware workgroup ids), 17 ntg (tap-row groups), 18 pixel tiles in all (ksplit never
 *    exceeds it). */
#define SOS_WGRAD_DESCRIBE_N 19
int sos_wgrad_describe(const sos_wgrad_desc* desc, int32_t* out, int n_out);

/* ---- backward of the BatchNorm(+activation) / bias(+activation) tail of a conv block (autograd of
 * nn.BatchNorm2d + ReLU/PReLU in train mode).  dy: grad of the block output; x: raw conv output;
 * scale/shift/mean/invstd: from sos_bn_finalize (mean == invstd == NULL: no BatchNorm);
 * partial: f32 scratch of 3 * C * sos_bn_stats_blocks(npix) floats; coef: f32 [4][C] scratch.  Writes dgamma, dbeta
 * (or the bias gradient), dslope[0] (PReLU) and dx = grad of the raw conv output. */
int sos_bn_bwd(const sos_view* dy, const sos_view* x, const float* scale, const float* shift, const float* mean,
               const float* invstd, const float* gamma, int act, const float* slope, float* partial, float* coef,
               float* dgamma, float* dbeta, float* dslope, const sos_view* dx,
               const float* out_scale /* optional device scalar: dgamma, dbeta, dslope are multiplied by it */,
               sos_stream_t stream);
/* dz = dy * act'(y) from the stored OUTPUT y (Linear+ReLU / Linear+Sigmoid heads). */
int sos_act_bwd_from_y(const sos_view* dy, const sos_view* y, int act, const sos_view* dz, sos_stream_t stream);
/* f32 strided gradient (x sigmoid'(y) if act == SOS_ACT_SIGMOID) -> bf16 rows: element (o,t,c) read at
 * g[o*so + t*st + c*sc], written to row o*inner+t, channel c of `out`. */
int sos_pack_grad_f32(const float* g, const float* y, int act, int64_t outer, int64_t inner, int C, int64_t so,
                      int64_t st, int64_t sc, const sos_view* out, const float* mul /* optional device scalar */,
                      sos_stream_t stream);
/* gradient of the LSTM feature matrix back to NHWC (inverse of the feature form of sos_bn_act_apply):
 * out[b][h][w][c] = sum_{i in [lo[w],hi[w])} feat[b][i][(feat.c_off+c)*H + h]  (lo/hi NULL: i == w). */
int sos_feat_to_nhwc(const sos_view* feat, int B, int H, int W, int Wo, const int32_t* lo, const int32_t* hi,
                     const sos_view* out, sos_stream_t stream);
/* ---- BPTT of the recurrent part of nn.LSTM (autograd of M1/networks.py:148, M2/networks.py:88).
 * dh_out: bf16 grad of the LSTM output [B][T][dh_cs] (dh_cs % 4 == 0); gates/csave from the forward;
 * wtk_hi / wtk_lo: the backward arrays of sos_lstm_pack_whh; dgates f32 [B][T][2][4H] (gate
 * pre-activation grads, gate-interleaved like xproj; dW_ih, dW_hh, bias and input grads are GEMMs over it). */
int sos_lstm_bidir_bwd(const void* dh_out, int dh_cs, int dh_dtype, int64_t dh_third, const float* gates,
                       const float* csave, const void* wtk_hi, const void* wtk_lo /* optional */, int64_t B, int64_t T,
                       int H, float* dgates, sos_stream_t stream);
/* ---- losses (M2/agent.py:174,188-189; M1/agent.py:187,202) and optimizer (M1/agent.py:177). */
int sos_mse_loss(const float* a, const float* b, int64_t n, float upstream, float* loss, float* grad, float* partial,
                 sos_stream_t stream);
int sos_bce_logits_loss(const float* x, const float* y, int64_t n, float upstream, float* loss, float* grad,
                        float* partial, sos_stream_t stream);
/* ---- loss scale of the fp16 storage mode (the reference trains in fp32, M2/agent.py:101-106; half precision needs
 * the gradients of the activations moved into its exponent range).  The scale is a power of two chosen ON THE DEVICE
 * from the gradient entering the hand-written backward, so no host synchronisation: sos_amax_f32 folds max|g| into
 * *amax (caller zeroes it; several tensors may be folded), sos_loss_scale writes scale2 = {S, 1/S} with
 * S = 2^floor(log2(target / amax)) clamped to [2^-40, 2^40] (S = 1 when amax is 0 or >= 3e38).  The backward multiplies S in
 * where f32 gradients become 16-bit (sos_pack_grad_f32 / sos_pack_nchw_to_nhwc `mul`) and 1/S where parameter
 * gradients leave (sos_wgrad_desc.scale_dev, sos_bn_bwd out_scale, sos_scale_f32): exact, the pass is linear. */
int sos_amax_f32(const float* x, int64_t n, float* amax, sos_stream_t stream);
int sos_loss_scale(const float* amax, float target, float* scale2, const float* guard /* optional: SOS_GUARD state, the
                   target is multiplied by its back-off factor */, sos_stream_t stream);
int sos_scale_f32(float* x, int64_t n, const float* s /* device scalar */, sos_stream_t stream);
/* ---- overflow guard of a training step (no counterpart in the reference, which trains in fp32: M2/agent.py:101-106;
 * the analogue of torch.cuda.amp.GradScaler's found_inf / skipped step, decided ON THE DEVICE: no host sync).
 * guard: device f32 [SOS_GUARD_FLOATS], zero-initialised by the caller once per model:
 *   [0] found  : 1 if the gradients checked last were not all finite, else 0 -- the optimizer kernels skip their whole
 *                update (parameters, exp_avg, exp_avg_sq untouched) while it is 1
 *   [1] backoff: factor in (0, 1] applied to sos_loss_scale's target (0 reads as 1): halved by every overflow (floor 2^-20),
 *                doubled again after SOS_GUARD_GROWTH consecutive finite steps
 *   [2] finite steps since the last change of [1];  [3] steps skipped so far;  [4] scratch (raw flag bits)
 * sos_grad_guard scans g[0..n) (a flat gradient buffer of the model, after the all-reduce) into the scratch flag and, when
 * `finalize` is non-zero, updates the state from it (several buffers: finalize with the last one). */
#define SOS_GUARD_FLOATS 5
#define SOS_GUARD_GROWTH 200
int sos_grad_guard(const float* g, int64_t n, float* guard, int finalize, sos_stream_t stream);
/* skip: optional device pointer to the guard state: a non-zero [0] turns the launch into a no-op, and once [3] (steps skipped so
 * far) is non-zero the bias corrections are taken at step - [3], the number of updates actually APPLIED (`step` counts attempts;
 * torch.cuda.amp.GradScaler semantics: a skipped update does not advance the optimizer's step) */
int sos_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, float grad_scale, const float* skip, sos_stream_t stream);

/* multi-tensor form: one launch for all parameter tensors of a model.  tensors: DEVICE array; chunks: DEVICE int32
 * [n_chunks][2] = (tensor index, chunk index), SOS_ADAM_CHUNK elements per chunk, covering every tensor. */
#define SOS_ADAM_CHUNK 16384
typedef struct sos_adam_tensor { float* p; const float* g; float* m; float* v; int64_t n; } sos_adam_tensor;
int sos_adam_multi_step(const sos_adam_tensor* tensors, int n_tensors, const int32_t* chunks, int64_t n_chunks, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                        const float* skip /* optional, see sos_adam_step */, sos_stream_t stream);

/* Re-pack every 16-bit weight tensor of a model from its fp32 parameters in ONE launch (after an optimizer step).
 * entries: DEVICE array; entry e fills out[0..n) (16-bit storage type) from idx[0..n) (device int64): idx > 0 = absolute
 * address of the fp32 source element, idx < 0 = the low part of the value at -idx (hi|lo|hi thirds of the three-pass
 * mode), 0 = zero padding.  chunks as for sos_adam_multi_step (SOS_ADAM_CHUNK elements each). */
typedef struct sos_pack_entry { const int64_t* idx; void* out; int64_t n; } sos_pack_entry;
int sos_gather_pack_multi(const sos_pack_entry* entries, int n_entries, const int32_t* chunks, int64_t n_chunks,
                          sos_stream_t stream);

/* backward of ReflectionPad2d(pad) (DownConvBlock, M2/networks.py:105): out (+)= fold of the padded-domain
 * gradient `padded` ([B][H+2pad][W+2pad]) onto the [B][H][W] interior. */
int sos_reflect_fold(const sos_view* padded, int H, int W, int pad, const sos_view* out, int accumulate,
                     sos_stream_t stream);
/* second half of a convolution launched with sos_conv_desc.fold_pad: out += the BORDER cells of `padded` folded onto the
 * interior cells they mirror (the interior cells were written by the convolution itself).  Touches only the pixels of `out`
 * within `pad` of an edge and the border of `padded`. */
int sos_reflect_fold_border(const sos_view* padded, int H, int W, int pad, const sos_view* out, sos_stream_t stream);
/* copy a channel slice between NHWC grids [B][Hs][Ws] -> [B][Hd][Wd]: overlap copied, rest of dst zeroed
 * (the crop that stands in for F.interpolate(out, skip.size()) at M2/networks.py:199-203, and its backward). */
int sos_copy_crop(const sos_view* src, int Hs, int Ws, const sos_view* dst, int Hd, int Wd, sos_stream_t stream);

/* ---- 8f-2  the wave front door: `librosa.load(path, sr=14000)` at M1/dataset.py:226, M2/predict.py:288,297,303
 * (soundfile decode -> to_mono -> resampy 'kaiser_best' -> fix_length) and the samples handed to
 * `librosa.output.write_wav` (M2/predict.py:515-528).  The RIFF container is parsed on the host; these take the
 * decoded, still interleaved samples. */
enum { SOS_PCM_S16 = 0, SOS_PCM_S32 = 1, SOS_PCM_F32 = 2, SOS_PCM_U8 = 3 };
/* pcm: interleaved [n_frames][channels] device samples -> out f32 [n_frames] = mean over channels of
 * sample / 2^(bits-1) (u8: (v-128)/128; f32: as is). */
int sos_pcm_to_mono_f32(const void* pcm, int format, int channels, int64_t n_frames, float* out, sos_stream_t stream);
/* The same decode WITHOUT the mix-down, and its inverse, for a group of files in one launch each (csrc/pcm_io.hip;
 * sos_amd.audio_io.decode_planes_batch_device / encode_batch_device; float64 restatement: tests/pcm_reference.py).  Both follow
 * the ragged conventions below (sos_ragged_stage_f32): an int64 table in two copies, table on the device and table_host on the
 * HOST; the host validates its own copy before any launch, the kernels follow the device copy and skip a row that does not lie
 * inside the totals the host summed.  1 .. 65535 files per call.
 * sos_pcm_planes_batch_f32: pcm = the interleaved [frames][channels] samples of files that share one SOS_PCM_* format, back to
 *   back.  Row per file, int64 [nfiles][4] = {element offset into pcm, frames, channels (1 .. 64), first output sample}; files
 *   lie in table order without overlap on both sides.  out: f32 channel planes, channel c of file f at out[row.out + c * frames
 *   .. + frames), every value bit for bit sample / 2^(bits-1) as sos_pcm_to_mono_f32 converts it (one channel: the same bits).
 * sos_pcm_encode_batch: planes = f32 channel planes.  Row per file, int64 [nfiles][5] = {first plane sample, plane length
 *   available, channels (1 .. 64), frames to write, output ELEMENT offset}: channel c is planes[row.first + c * available ..
 *   + available).  out: interleaved [frames][channels] per file in `format`, files back to back in table order; an element is
 *   2 / 3 / 4 / 1 / 4 bytes for SOS_ENC_S16 / S24 (packed, little-endian) / S32 / U8 / F32.  Per sample: x = the plane's value
 *   below `available`, 0 from there to `frames` (crop and zero-fill happen here); F32 copies the bits; otherwise q =
 *   rint((double)x * S) half to even with S = 2^15 / 2^23 / 2^31 / 2^7, NaN -> 0, saturated to [-S, S - 1]; U8 stores q + 128.
 *   clipped: int64 [nfiles], set by the call to the number of the file's samples that were NaN or changed by saturation
 *   (+-inf included; 0 for F32).  No dither.  No byte outside a file's frames * channels * width bytes is written.
 * SOS_EINVAL (sos_last_error() names the file): null pointers, nfiles outside 1 .. 65535, an unknown format, channels outside
 * 1 .. 64, negative frames / available, or a row that overlaps its predecessor or lies outside the totals. */
enum { SOS_ENC_S16 = 0, SOS_ENC_S32 = 1, SOS_ENC_F32 = 2, SOS_ENC_U8 = 3, SOS_ENC_S24 = 4 };
int sos_pcm_planes_batch_f32(const void* pcm, int format, const int64_t* table, const int64_t* table_host, int nfiles, float* out,
                             sos_stream_t stream);
int sos_pcm_encode_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int format, void* out,
                         int64_t* clipped, sos_stream_t stream);
/* G.711 (ITU-T G.711: A-law, WAVE format tag 6, and mu-law, tag 7; one code byte per sample) through the same kernels
 * (csrc/pcm_core.h states the rule once, in integers and without a table; float restatement: tests/g711_reference.py, held
 * against the Sun / ITU g711.c as CPython's audioop carries it, on all 256 codes and all 65 536 s16 values).  The rule is
 * stateless per sample, so a live leg's packets go through the same calls as files.
 * Expand, code c -> level, value = level / 32768 as f32 (exact):
 *   mu-law: u = ~c & 0xFF; t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7); level = u & 0x80 ? 0x84 - t : t - 0x84   (+-32124)
 *   A-law:  a = c ^ 0x55; seg = (a >> 4) & 7; t = (a & 15) << 4;
 *           t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1); level = a & 0x80 ? t : -t                                (+-32256)
 * Compress, f32 x -> code: q = the SOS_ENC_S16 value of x (rint half to even in double, NaN -> 0, saturated; `clipped` counts
 * exactly what it counts for S16), then the reference compressor, which DROPS the low bits (it does not round to the nearest
 * level; what audioop, libsndfile and sox write):
 *   mu-law: p = q >> 2; mask = p < 0 ? 0x7F : 0xFF; p = min(|p| + 0x21, 0x1FFF); seg = index of the first of the ends
 *           {0x3F, 0x7F, .. 0x1FFF} that is >= p; code = ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ mask
 *   A-law:  p = q >> 3; mask = p < 0 ? 0x55 : 0xD5; if p < 0: p = -p - 1; seg over the ends {0x1F, 0x3F, .. 0xFFF};
 *           code = ((seg << 4) | ((p >> max(seg, 1)) & 15)) ^ mask
 * Expanding and compressing again returns every code except mu-law 0x7F (negative zero), which comes back as 0xFF.  Silence
 * is 0xFF (mu-law) / 0xD5 (A-law): the zero-fill past a plane's end is the float 0 compressed, hence that code, never byte 0.
 * sos_g711_planes_batch_f32 / sos_g711_encode_batch / sos_g711_to_mono_f32: sos_pcm_planes_batch_f32 / sos_pcm_encode_batch /
 * sos_pcm_to_mono_f32 with `law` in place of the format and one byte per element: the same tables, bounds rule, refusals
 * (an unknown law: SOS_EINVAL, "unknown law %d") and mean expression. */
enum { SOS_G711_ALAW = 6, SOS_G711_ULAW = 7 };
int sos_g711_planes_batch_f32(const void* codes, int law, const int64_t* table, const int64_t* table_host, int nfiles, float* out,
                              sos_stream_t stream);
int sos_g711_encode_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int law, void* out,
                          int64_t* clipped, sos_stream_t stream);
int sos_g711_to_mono_f32(const void* codes, int law, int channels, int64_t n_frames, float* out, sos_stream_t stream);
/* sos_pcm_encode_batch with dither added before the rounding, for SOS_ENC_U8 / S16 / S24 (csrc/dither_core.h states the rule
 * once; numpy restatement: tests/dither_reference.py, exact, so the tests ask for equal bytes).  The dither of a sample is a pure
 * function of (seed, file key, channel, absolute frame), evaluated inside the encode kernels: a file's bytes do not depend on
 * the other files of the launch, on the grid or on the access path, and a signal encoded packet by packet, frame0 advanced by
 * each packet's length, gives the bytes of the signal encoded at once.
 * Row per file, int64 [nfiles][7]: the five columns of sos_pcm_encode_batch, then {file key (0 .. 2^32 - 1), frame0 = the absolute
 * frame of the file's first frame (0 .. 2^62 - frames)}; the same row checks and grid.
 * Generator: Philox4x32-10 (Salmon et al., Random123): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, round c' = {hi(M1 * c2) ^ c1
 *   ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)}, the key bumped by {0x9E3779B9, 0xBB67AE85} after each of ten rounds.
 * Word of a sample: n = frame0 + i; counter {low32(n >> 2), high32(n >> 2), channel, file key}, key {low32(seed), high32(seed)};
 *   w(n) = output word n & 3 of that block.
 * Dither in LSB: SOS_DITHER_TPDF d = ((w & 0xFFFF) - (w >> 16)) / 65536 (triangular on (-1, 1), variance 1/6);
 *   SOS_DITHER_HIGHPASS d[n] = (u(n + 1) - u(n)) / 65536 with u(n) = w(n) & 0xFFFF (the same marginal, its spectrum (1/12)(2 - 2 cos w)
 *   moved towards fs / 2; it shapes the dither only, the quantisation error is not fed back).
 * q = rint((double)x * S + d) half to even, then as sos_pcm_encode_batch: NaN -> 0, saturated to [-S, S - 1]; `clipped` counts
 *   after the dither (it can push a sample at the ceiling over it).  Every written sample is dithered, the zero-fill past the
 *   plane's end included.
 * SOS_EINVAL beyond sos_pcm_encode_batch's: a dither other than the two, SOS_ENC_S32 / SOS_ENC_F32 / a G.711 law (S32 holds more
 * bits than a float's mantissa, F32 is a copy, G.711 drops the low bits of the s16 value), a key or frame0 outside its range. */
enum { SOS_DITHER_TPDF = 1, SOS_DITHER_HIGHPASS = 2 };
int sos_pcm_encode_dither_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int format,
                                int dither, uint64_t seed, void* out, int64_t* clipped, sos_stream_t stream);
/* Integrated loudness (ITU-R BS.1770-4 / EBU R128) of a group of files on the planes sos_pcm_encode_batch reads, and the gain
 * that brings each file to a target (csrc/loudness.hip; sos_amd.metrics.loudness_batch / audio_io.loudness_gain_batch_device;
 * float64 restatement: tests/loudness_reference.py).  The ragged conventions of the entry points above: the table in two
 * copies, the host validates its own before any launch, the kernels skip a device row outside the totals the host summed.
 * Row per file, int64 [nfiles][8] = the encode row {first plane sample, plane length available, channels (1 .. 64), frames,
 * (the output offset: not read)}, then {hop h = (rate + 5) / 10 samples, index of the file's first channel weight, index of the
 * file's first chunk}; a file has channels * ceil(frames / h) * split chunks, files in table order.  A sample is the plane's
 * value below `available` and 0 from there to `frames`, as the encode reads it.
 * sos_loudness_batch_f64: coef f64 [nfiles][10] = {b0, b1, b2, a1, a2} of the two K-weighting biquads at the file's rate
 *   (sos_amd.metrics.k_weighting; transposed direct form II, zero initial state), weights f64 [sum of channels].  Blocks of 4 h
 *   samples every h, whole blocks only: z = sum_c w_c mean(y_c^2), l = -0.691 + 10 log10 z; gates l > -70 and l > (loudness of
 *   the absolutely gated blocks) - 10.  stats f64 [nfiles][4] = {L = -0.691 + 10 log10(mean z of the blocks passing both), -inf
 *   without one; max |x| over all channels and frames (the SAMPLE peak); blocks passing both gates; blocks passing the absolute
 *   one}, {NaN, NaN, -1, -1} for a skipped row.  The filter is evaluated as a chunked linear recurrence, `split` (1 .. 64, at
 *   most h) chunks per hop; every operation after the load is float64 and every sum has a fixed order.  work: device bytes,
 *   at least sos_loudness_workspace_bytes(table_host, nfiles, split) (-1 for a table the call would refuse); SOS_ENOSPC below it.
 * sos_loudness_gain_batch_f32: per file g = min(10^((targets[f] - L) / 20), 10^(ceiling_db / 20) / peak) in double from
 *   stats[f], stored as f32; g = 1 where L, the peak or the target give none (L = -inf, peak 0, not finite).  Scales the first
 *   min(frames, available) samples of every channel IN PLACE, x * g in f32; writes gains f32 [nfiles] and limited int32
 *   [nfiles] (1: the ceiling bound the gain).  Reads columns 0 .. 3 of the table only.  ceiling_db > 0 is refused.
 * SOS_EINVAL (sos_last_error() names the file): null pointers, nfiles outside 1 .. 65535, split outside 1 .. 64, channels
 * outside 1 .. 64, negative frames / available, a hop below 1 or below split, or a row outside the totals. */
int64_t sos_loudness_workspace_bytes(const int64_t* table_host, int nfiles, int split);
int sos_loudness_batch_f64(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, const double* coef,
                           const double* weights, int split, void* work, int64_t work_bytes, double* stats, sos_stream_t stream);
int sos_loudness_gain_batch_f32(float* planes, const int64_t* table, const int64_t* table_host, int nfiles, const double* stats,
                                const double* targets, double ceiling_db, float* gains, int* limited, sos_stream_t stream);
/* The other EBU R128 measures of a group of files, on the table above (csrc/loudness.hip; sos_amd.metrics.true_peak_batch /
 * loudness_batch(true_peak=, loudness_range=); float64 restatement: tests/r128_reference.py).  No call waits for the device.
 * sos_true_peak_batch_f64: the true peak (ITU-R BS.1770-4 Annex 2) by the project's own interpolator, 4x oversampling by a
 *   48-tap polyphase windowed sinc.  Reads columns 0 .. 3 of the table only; the host checks are sos_loudness_gain_batch_f32's.
 *   coef f32 [3][12] on the device (sos_amd.metrics.true_peak_filter): h_p[k] = sinc(u) I0(9 sqrt(1 - (u / 6)^2)) / I0(9), u =
 *   k - p / 4, for p = 1, 2, 3 and k = -5 .. 6, computed in double and rounded once.  The point n + p / 4 is v = sum_k h_p[k]
 *   x[n + k], 12 fmaf in tap order in f32, for n = -1 .. frames - 1; phase 0 is the sample; x reads 0 outside [0, min(frames,
 *   available)).  peaks f64 [nfiles] = max over channels of |x| and |v| (the f32 maximum, widened; the type of column 1 of the
 *   stats rows), 0 for a file without a sample, NaN for a skipped row.  Two launches (peaks are initialised on the stream); the
 *   grid is flat over tiles of 2048 points of all planes; a maximum has no order: two calls give equal bits.
 * sos_loudness_range_batch_f64: work = the buffer sos_loudness_batch_f64 filled on the same stream with the same table,
 *   weights and split.  e[i] = sum_c w_c (sum of y_c^2 over hop i), whole hops only; short-term windows of 30 hops every hop:
 *   z[j] = (e[j] + .. + e[j + 29]) / (30 h), l = -0.691 + 10 log10 z; gates l > -70 and l > (loudness of the mean z of the
 *   absolutely gated windows) - 20; with s the m surviving l ascending, LRA = s[floor((m - 1) 0.95 + 0.5)] - s[floor((m - 1) 0.10
 *   + 0.5)] (EBU Tech 3342 by libebur128's nearest ranks), 0 for m = 0.  out f64 [nfiles][4] = {LRA in LU, maximum momentary
 *   loudness (400 ms blocks, ungated, -inf without one), maximum short-term loudness (ungated, -inf without a window), m},
 *   {NaN, NaN, NaN, -1} for a skipped row.  range_work: device bytes, at least sos_loudness_range_workspace_bytes(table_host,
 *   nfiles) (16 bytes per hop of every plane, whatever the split; -1 for a table the call would refuse); SOS_ENOSPC below it
 *   or with a work buffer below sos_loudness_workspace_bytes.  Two launches.
 * SOS_EINVAL as above. */
int sos_true_peak_batch_f64(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, const float* coef,
                            double* peaks, sos_stream_t stream);
int64_t sos_loudness_range_workspace_bytes(const int64_t* table_host, int nfiles);
int sos_loudness_range_batch_f64(const int64_t* table, const int64_t* table_host, int nfiles, const double* weights, int split,
                                 const void* work, int64_t work_bytes, void* range_work, int64_t range_work_bytes, double* out,
                                 sos_stream_t stream);
/* The look-ahead limiter on the table above (csrc/limiter.hip; sos_amd.audio_io.limit_batch_device; float64 restatement:
 * tests/limiter_reference.py): every file at the gain s that brings it to its target, its peaks held at the ceiling by ONE gain
 * curve g[t] <= 1 for all its channels.  Reads columns 0 .. 4 of the table: column 4 is H, the look-ahead in samples (1 .. 1024).
 * With m = min(frames, available), samples outside [0, m) reading 0: s = (float)10^((targets[f] - L) / 20) in double from
 * stats[f] (1 where L or the target is not finite), C = (float)10^(ceiling_db / 20); p[t] = max over channels of |x[t]|, with
 * true_peak != 0 also of the six interpolated points next to t (t - 1 + q / 4 and t + q / 4, q = 1, 2, 3: the points of
 * sos_true_peak_batch_f64, coef as there; coef may be null otherwise); a = s * p[t] in f32, r[t] = a > C ? max((float)((double)C /
 * (double)a), 2^-10) : 1, r = 1 outside [0, m); mn[t] = min r[t - H .. t + H]; g[t] = (float)(sum of (double)mn[t - H .. t + H] /
 * (2 H + 1)) -- every mn is a multiple of 2^-33, the float64 sum is exact in any order; out[t] = x[t] * (g[t] * s) for t < m, and
 * the samples [m, available) are copied.  g[t] <= r[t]; where g = 1 the output is what sos_loudness_gain_batch_f32 writes with
 * the gain s.  `out` has the layout of `planes` and may not overlap it.  rows f64 [nfiles][4] = {s, min g, samples with g < 1,
 * 0}, {NaN, NaN, -1, 0} for a skipped row; the minimum and the count are atomics without an order: two calls give equal bits.
 * Three launches (the grid is flat over tiles of SOS_LIMITER_TILE samples of all files), no wait.
 * SOS_EINVAL as above, and: H outside 1 .. 1024, a ceiling above 0 or not finite, out overlapping planes. */
#define SOS_LIMITER_TILE 4096
int sos_limiter_batch_f32(const float* planes, float* out, const int64_t* table, const int64_t* table_host, int nfiles,
                          const double* stats, const double* targets, double ceiling_db, int true_peak, const float* coef,
                          double* rows, sos_stream_t stream);
/* Band-limited resampling by `ratio` = sr_new / sr_orig (resampy 0.2.2 `resample_f`): win = the filter's half
 * window (nwin floats, num_table samples per zero crossing), already multiplied by min(1, ratio).  Writes
 * out[0 .. n_out): the first floor(n_in * ratio) entries are resampled, the rest zero (librosa pads to
 * ceil(n_in * ratio)).  (nwin + 1) * 4 bytes must fit the 160 KB LDS. */
int sos_resample_f32(const float* x, int64_t n_in, double ratio, const float* win, int nwin, int num_table,
                     float* out, int64_t n_out, sos_stream_t stream);
/* sos_resample_f32 for a ragged batch of clips at one common ratio, in ONE launch whatever nclips is
 * (csrc/wave_io.hip resample_batch_kernel: one workgroup per CU walks the (clip, SOS_RESAMPLE_CHUNK outputs) tiles).  x: the clips back to back in one f32 buffer; out: one
 * buffer for all outputs, not pre-cleared.  table: int64 [6][nclips] on the device, table_host: the same values on the
 * HOST (they are validated there before anything touches the device, and size the grid):
 *   [0] input offset   [1] n_in   [2] output offset   [3] n_out   [4] n_valid = min((int64)(n_in * ratio), n_out)
 *   [5] the clip's first tile = sum of ceil(n_out / SOS_RESAMPLE_CHUNK) over the clips before it
 * Clips lie in increasing order of both offsets and do not overlap.  Clip c gets, bit for bit, what sos_resample_f32 writes
 * for that clip alone -- in any batch and any order: every bound is the clip's own, no tap reads a neighbour, outputs
 * n_valid .. n_out are written as zero.  A device entry that lies outside what table_host sized is skipped.
 * SOS_EINVAL (sos_last_error() names the clip): null pointers, nclips outside 1 .. 65535, n_in < 1, n_valid < 1 or not the
 * value above, ratio <= 0, (nwin + 1) * 4 bytes > 160 KB; SOS_ENOSPC: the time register of the longest clip needs more
 * segments than the kernel argument holds. */
#define SOS_RESAMPLE_CHUNK 4096
int sos_resample_batch_f32(const float* x, const int64_t* table, const int64_t* table_host, int nclips, double ratio,
                           const float* win, int nwin, int num_table, float* out, sos_stream_t stream);
/* Host-only helper (no GPU work): the piecewise-linear description of resampy's running f64 time register
 * `time_register += 1/ratio` that sos_resample_f32 hands its kernel: time(t) = fma(t - k0[i], d[i], s0[i]) for
 * the last i with k0[i] <= t.  Returns the number of segments (<= capacity) or a negative error. */
int sos_resample_time_segments(double ratio, int64_t n_out, int64_t* k0, double* s0, double* d, int capacity);
/* The band above the networks' half rate (csrc/band_merge.hip; sos_amd.audio_io.band_gains_batch_device /
 * resample_merge_batch_device; float64 restatement: tests/band_reference.py).  Per channel of a recording whose rate R exceeds
 * the networks' SR: x = the native plane, n frames; a = x resampled to SR, m = ceil(n * SR / R) samples; b = the networks'
 * output for a, m' <= m samples (hop * (m / hop)); ratio = R / SR; U(v) = what sos_resample_f32 writes for v at `ratio`
 * (resampled for t < (int64)(len(v) * ratio), zero after).  The rule, all f32:
 *     out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t])        0 <= t < n
 * U(b) is what resampling the networks' output back gives; g * (x - U(a)) is the part of the source the SR chain never saw.
 * Both follow the ragged conventions (table on the device, table_host on the HOST, validated there before any launch; the
 * kernels skip a device row that fails the same bounds); 1 .. 65535 clips per call, every signal's clips back to back in its own
 * buffer, in table order without overlap.
 * sos_band_gain_batch_f32: table int64 [6][nclips] = [0] a offset [1] m [2] b offset [3] m' (0 .. m) [4] gains offset
 *   [5] J = ceil(m / hop).  Frame j covers the samples [j hop, (j + 1) hop) cut at m; E_a[j] = sum a^2, E_b[j] = sum b^2 in
 *   f64 (no fixed order), b reading zero from m' on; r[j] = 1 if E_a[j] == 0, else min(1, sqrt(E_b[j] / E_a[j])); gains[j] =
 *   s[j] = the f64 mean of r[max(0, j - smooth) .. min(J - 1, j + smooth)], stored as f32.  One launch.
 * sos_resample_merge_batch_f32: table int64 [9][nclips] = [0] offset of the clip in x and in out [1] n [2] a offset [3] m
 *   [4] b offset [5] m' (1 .. m) [6] gains offset [7] J [8] the clip's first tile = sum of ceil(n / SOS_RESAMPLE_CHUNK) over the
 *   clips before it.  One launch whatever nclips is (one workgroup per CU walks the (clip, SOS_RESAMPLE_CHUNK outputs) tiles, as
 *   sos_resample_batch_f32 does).  U(a)[t] and U(b)[t] carry the bits of sos_resample_f32 (the same taps in the same order, each
 *   signal's right wing ending at its own last sample).  gains == NULL: g = 1 and rows [6], [7] are not read; otherwise g[t] =
 *   the linear interpolation of the clip's s[0 .. J) at the frame-centre position p = (t + 0.5) / (ratio * hop) - 0.5, s[0] for
 *   p <= 0 and s[J - 1] for p >= J - 1, evaluated in f64 and rounded to f32.  out is not pre-cleared; exactly n floats are
 *   written per clip.
 * SOS_EINVAL (sos_last_error() names the clip): null pointers (gains may be NULL for the merge), nclips outside 1 .. 65535,
 * hop < 1, smooth outside 0 .. 16, m < 1, m' outside its range, J not ceil(m / hop), spans that overlap or are out of order;
 * for the merge also n < 1, (int64)(m * ratio) < n (U(a) would not cover the clip), a wrong first tile, ratio <= 0,
 * (nwin + 1) * 4 bytes > 160 KB; SOS_ENOSPC: the time register of the longest clip needs more segments than the kernel
 * argument holds. */
int sos_band_gain_batch_f32(const float* a, const float* b, const int64_t* table, const int64_t* table_host, int nclips, int hop,
                            int smooth, float* gains, sos_stream_t stream);
int sos_resample_merge_batch_f32(const float* x, const float* a, const float* b, const float* gains, const int64_t* table,
                                 const int64_t* table_host, int nclips, double ratio, const float* win, int nwin, int num_table,
                                 int hop, float* out, sos_stream_t stream);

/* ---- 8f-1  audio-visual variant, video branch: Conv3dBlock M1/networks.py:54-77, make_video_branch :110-118
 * (configuration :87-89), fusion :135-142.  A Conv3d with temporal stride 1 runs on sos_conv2d_fwd over a
 * time-stacked input (temporal taps on the contraction axis).
 * sos_time_stack: in bf16 [B*T][HW][nseg*in_cs] (C real channels per third) -> out [B*T][HW][nseg*out_cs] with
 *   out channel dt*C + c = frame t + dt - (kt-1)/2, zeros outside the clip and in the padding (out_cs >= kt*C).
 * sos_spatial_mean: torch.mean(f_v, dim=(-2,-1)) of N images into out[n*out_row + third*out_third + out_c_off + c]. */
int sos_time_stack(const void* in, int64_t B, int T, int64_t HW, int C, int in_cs, int nseg, int kt, void* out,
                   int out_cs, sos_stream_t stream);
int sos_spatial_mean(const void* in, int64_t N, int64_t HW, int C, int in_cs, int nseg, void* out, int64_t out_row,
                     int out_third, int out_c_off, sos_stream_t stream);
/* their transposes (autograd of the variant): gradient of the stacked tensor folded back onto the frames, and the
 * gradient of the spatial mean broadcast over the HW pixels (hi|hi|lo thirds re-split in bf16x3 mode). */
int sos_time_unstack(const void* d_stacked, int64_t B, int T, int64_t HW, int C, int st_cs, int nseg, int kt,
                     void* d_in, int in_cs, sos_stream_t stream);
int sos_spatial_mean_bwd(const void* dfeat, int64_t N, int64_t HW, int C, int64_t f_row, int f_third, int f_c_off,
                         int nseg, void* dy, int cs, sos_stream_t stream);

/* ---- 8f-4  objective measures of M2/metrics.py, the per-sample / per-frame work (finalisation = host code in
 * sos_amd/metrics.py): f32 device signals, frames start = f*skip of `winlength` samples under `window` (f64[winlength]).
 * sos_metric_totals      : out3 = {sum ref^2, sum (ref-deg)^2, max |ref|}            (overall SNR :97, silence threshold :192)
 * sos_metric_frame_energy: out[f] = {sum (w c)^2, sum (w c - w p)^2}                (metrics_ssnr* :119-127)
 * sos_metric_compact     : keeps, in order, the samples with |clean| >= thr         (metrics_ssnr_exclude_silence :189-199)
 * sos_metric_llr         : out[f] = log(a_p R_c a_p' / a_c R_c a_c'), order-P LPC   (llr :561-623, lpcoeff :626-681)
 * sos_metric_wss         : out[f] = weighted spectral slope distance, crit_filter f32 [25][n_fft/2]   (wss :404-558)
 * sos_metric_l1          : mean |lerp(output)(linspace(0, n_out-1, n_t)) - target|  (metrics_L1 :40-45) */
int sos_metric_totals(const float* ref, const float* deg, int64_t n, double* out3, sos_stream_t stream);
int sos_metric_frame_energy(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                            const double* window, double* out, sos_stream_t stream);
int sos_metric_compact(const float* clean, const float* proc, int64_t n, float thr, float* out_clean, float* out_proc,
                       int64_t* count, sos_stream_t stream);
int sos_metric_llr(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                   const double* window, int P, float* out, sos_stream_t stream);
int sos_metric_wss(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                   const double* window, int n_fft, const float* crit_filter, double eps, float* out, sos_stream_t stream);
int sos_metric_l1(const float* output, int64_t n_out, const float* target, int64_t n_t, double* result, sos_stream_t stream);

/* ---- 8f-4  the measures above for a ragged batch of (clean, noisy) pairs in one launch sequence (csrc/metrics_batch.hip;
 * sos_amd.metrics.evaluate_metrics_batch): no allocation, no host synchronisation, and every value of a clip depends on that
 * clip's samples only.  clean, noisy, offsets, lengths, lengths_host: as sos_stoi_batch (clip b is clean[offsets[b] ..
 * offsets[b] + lengths[b]); both buffers hold at least sum(lengths_host) samples).  winlength / skip / window as above,
 * n_fft a power of two >= 2 winlength, P the LPC order of LLR (<= 16), crit_filter f32 [25][n_fft/2], eps the floor of the
 * WSS band energies.  F_b = (long long)((double)n_b / skip - (double)winlength / skip), clamped at 0: the reference's frame
 * count in f64, which is NOT (n_b - winlength) / skip in integers (22050 Hz, n = 21122: 123 against 124).
 * sos_metric_batch_workspace_bytes: workspace size for these lengths (worst case: no sample removed), -1 on bad args.
 * sos_metric_batch: `out` is one packed buffer of 64 nclips + 40 Ftot bytes, Ftot = sum of F_b over lengths_host, frame-indexed
 * arrays in clip order (clip b at the sum of F_0 .. F_b-1):
 *   f64 [nclips][8]  {sum c^2, sum (c-n)^2, max |c|, sum |n-c|, kept samples k, kept frames, frames, status}
 *   f64 [Ftot][2]    frame energies {sum (w c)^2, sum (w c - w n)^2} of the full signals
 *   f64 [Ftot][2]    the same of the signals without the samples |c| < float(max |c|) * 0.03f; clip b's first
 *                    "kept frames" rows (the frame count of k, computed on the device) are written
 *   f32 [Ftot]       LLR per frame        f32 [Ftot]  WSS per frame (the values of sos_metric_llr / sos_metric_wss, bit for bit)
 * status = -1 (and zero frames): device lengths or offsets that overrun what lengths_host sized; the clip is not scored.
 * SOS_EINVAL with a message when a frame's LDS, (2 winlength + 3 n_fft) * 4 bytes, exceeds 60 KB. */
int64_t sos_metric_batch_workspace_bytes(const int64_t* lengths_host, int nclips, int winlength, int skip, int n_fft);
int sos_metric_batch(const float* clean, const float* noisy, const int64_t* offsets, const int64_t* lengths,
                     const int64_t* lengths_host, int nclips, int winlength, int skip, int n_fft, int P, const double* window,
                     const float* crit_filter, double eps, void* workspace, int64_t workspace_bytes, void* out, int64_t out_bytes,
                     sos_stream_t stream);

/* ---- 8f-4  STOI / extended STOI (Taal et al. 2011; Jensen & Taal 2016) of a ragged batch, pystoi's
 * stoi(x, y, fs_sig, extended) contract (float64 restatement: tests/stoi_reference.py; csrc/stoi.hip).
 * x, y: f32 clean / processed clips concatenated; clip b is x[offsets[b] .. offsets[b] + lengths[b]) (int64 device tables;
 * lengths_host: the same lengths on the HOST, which size the workspace and the grids).  p / q = 10000 / fs_sig reduced by
 * their gcd; for p != q, taps = f64 [ntaps] (ntaps = 2L+1 odd): Octave's resample filter normalised to unit sum and
 * multiplied by p (scipy.signal.resample_poly's window).  extended: 0 = classic STOI, 1 = ESTOI.
 * sos_stoi_workspace_bytes: workspace size for these lengths (worst case: no frame removed), -1 on bad args.
 * sos_stoi_batch: out f64 [nclips][3] = {sum of the per-segment correlations (fixed order), segments, kept frames}; the score
 * is sum / (segments * 15) (classic) or sum / segments (extended); segments = 0 means fewer than 30 STFT frames (pystoi
 * returns 1e-5); kept frames = -1: device lengths that overrun a workspace sized from lengths_host (not scored). */
int64_t sos_stoi_workspace_bytes(const int64_t* lengths_host, int nclips, int p, int q);
int sos_stoi_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths, const int64_t* lengths_host,
                   int nclips, int p, int q, const double* taps, int ntaps, int extended, void* workspace, int64_t workspace_bytes,
                   double* out, sos_stream_t stream);

/* ---- SI-SDR and the BSS-eval SDR of a ragged batch of (clean x, estimate y) pairs (csrc/sdr.hip; sos_amd.metrics.si_sdr_batch /
 * sdr_batch; float64 restatement: tests/sdr_reference.py).  x, y, offsets, lengths, lengths_host: as sos_stoi_batch; both buffers
 * hold at least sum(lengths_host) samples.  Every sum and the solve accumulate in f64 over fixed 4096-sample chunks in a fixed
 * order, without atomics: a clip's values depend on that clip's samples only.  No allocation, no host synchronisation.
 * sos_sdr_workspace_bytes: workspace size for these lengths, -1 on bad args; filter_length 0 sizes sos_sisdr_batch's workspace,
 *   1 .. 512 sos_sdr_batch's: 256-byte-aligned arrays of 40 nclips + 8200 C bytes, C = sum of ceil(n_b / 4096) (every chunk
 *   holds 512 lags of both correlations, whatever filter_length is).
 * sos_sisdr_batch: oracle/frontend.py::si_sdr's terms, on mean-removed signals when zero_mean = 1: out f64 [nclips][4] =
 *   {sum (alpha x)^2, sum (alpha x - y)^2, alpha = <y,x> / (<x,x> + 1e-30), samples}; alpha comes from sums over the mean-removed
 *   samples themselves (the means from a pass before), the residual from a further pass with the device's alpha; SI-SDR = 10 log10((out[0] + 1e-30) / (out[1] + 1e-30)).
 * sos_sdr_batch: r[k] = sum_t x[t] x[t+k], d[k] = sum_t x[t] y[t+k] for k < filter_length (1 .. 512), toeplitz(r) c = d by the
 *   Levinson-Durbin recursion: out f64 [nclips][5] = {p = d.c, e = sum y^2, r[0], status, samples}; SDR = 10 log10(p / (e - p)).
 *   status 0: solved; -2: r[0] <= 0 (an all-zero clean clip); -3: the prediction error stopped being positive (toeplitz(r) is
 *   numerically singular); p is 0 then.  stages: SOS_SDR_CORRELATE | SOS_SDR_SOLVE runs the sequence; one of the two runs that
 *   part alone (timing the two kernels apart): SOS_SDR_SOLVE then sums whatever the workspace holds, so it wants the same call
 *   with SOS_SDR_CORRELATE before it.  Either part first rebuilds the per-clip extents from this call's offsets / lengths, so
 *   no index it uses comes from the workspace's previous contents.
 * In both outputs samples = -1 (and status -1): device offsets / lengths that leave what lengths_host sized; the clip is not
 * scored.  SOS_EINVAL: null pointers, nclips outside 1 .. 65535, filter_length or stages out of range; SOS_ENOSPC: workspace
 * smaller than sos_sdr_workspace_bytes says. */
enum { SOS_SDR_CORRELATE = 1, SOS_SDR_SOLVE = 2 };
int64_t sos_sdr_workspace_bytes(const int64_t* lengths_host, int nclips, int filter_length);
int sos_sisdr_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths, const int64_t* lengths_host,
                    int nclips, int zero_mean, void* workspace, int64_t workspace_bytes, double* out, sos_stream_t stream);
int sos_sdr_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths, const int64_t* lengths_host,
                  int nclips, int filter_length, int stages, void* workspace, int64_t workspace_bytes, double* out,
                  sos_stream_t stream);

/* ---- ragged groups of clips: staging for the networks and unpacking of results (csrc/ragged_io.hip).  One launch each,
 * whatever the number of clips; no allocation, no host synchronisation.
 * sos_ragged_stage_f32: x = the clips back to back in one f32 buffer.  table: int64 [nclips][4] on the device,
 *   {sample offset, samples, bit offset, frames} per clip; table_host: the same values on the HOST (validated there, and they
 *   size the buffers: x and mask hold sum(samples) floats, bits holds sum(frames) bytes).  bits: the clips' frame decisions back
 *   to back (1 = non-silent); ratios / ratios_host: one double per clip on the device / the host, samples per frame
 *   (sr / framerate, > 1).  Writes wave [nclips][stride] = the clip, zero from its end to the stride; masked [nclips][stride] =
 *   clip * mask, zero-filled alike; mask = 1 on silent samples, back to back at the clip's sample offset.  A clip's mask is bit
 *   for bit what sos_bits_to_mask gives that clip alone at its ratio (csrc/mask_rule.h is the one statement of the rule), in
 *   any group and any order.  bits = NULL: only wave is written (ratios, masked, mask are not touched and may be NULL).
 * sos_ragged_unpack_f32: rows f32 [n_rows][stride]; table / table_host: int64 [nentries][3] = {row, valid samples, output
 *   offset}; out holds sum(valid) floats; out[offset .. offset + valid) = rows[row][0 .. valid).  Rows may repeat or be left
 *   out, entries may come in any order.
 * SOS_EINVAL (sos_last_error() names the entry): null pointers, nclips / nentries outside 1 .. 65535, stride < 1, samples or
 * valid > stride, a row outside n_rows, a ratio <= 1, or an entry that lies outside the samples / frames summed from the host
 * table.  The kernels follow the DEVICE table and skip an entry that fails the same bounds rule. */
int sos_ragged_stage_f32(const float* x, const int64_t* table, const int64_t* table_host, int nclips, const uint8_t* bits,
                         const double* ratios, const double* ratios_host, int64_t stride, float* wave, float* masked,
                         float* mask, sos_stream_t stream);
int sos_ragged_unpack_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table, const int64_t* table_host,
                          int nentries, float* out, sos_stream_t stream);

/* ---- silent-interval labels of clean speech for a ragged batch of clips (csrc/silence_label.hip; sos_amd.labels; float64
 * restatement: tests/silence_reference.py; parity with the reference's preprocessing/get_bitstream_better is unpinned).
 * x = the clips back to back in one f32 buffer.  table / table_host: int64 [nclips][4] on the device / the HOST, {sample offset,
 * samples, frame offset, frames} per clip -- the four columns of sos_ragged_stage_f32's table, so one table serves both calls
 * and `bits` goes into that call as it is.  params / params_host: f64 [nclips][5] on the device / the host, {ratio = samples per
 * frame (sr / framerate, > 1), rel = 10^(-threshold_db / 10), floor, min_silent, min_speech (frames, >= 1; 1 disables the pass)}.
 * Frame i of a clip of n samples is [int(i ratio), min(int((i+1) ratio), n)), the products rounded once in double; `frames`
 * must tile the clip: int((frames-1) ratio) < n <= int(frames ratio) (ceil(n / ratio) up to the rounding of the products).
 *   E[i] = mean of x^2 over frame i, f64, a fixed order that depends on the frame's own samples only (no atomics);
 *   quiet[i] = E[i] <= T, T = max(rel max_i E[i], floor);
 *   pass 1: a run of non-quiet frames shorter than min_speech with quiet frames on both sides turns quiet;
 *   pass 2: of the runs as pass 1 left them, a quiet run shorter than min_silent turns non-quiet, wherever it lies.
 * Writes bits [sum frames] (1 = non-silent, sos_bits_to_mask's convention) and energy f64 [sum frames] at the clips' frame
 * offsets, and out f64 [nclips][6] = {max E, T, silent frames, silent runs, frames, status}.  A clip's bits and energies are the
 * same alone, in any batch and in any order.  frames = -1 and status = -1: the DEVICE table or parameters leave what the host's
 * sized (the bounds rule of the other ragged kernels, and the tiling rule above); nothing is read or written for that clip.
 * Two launches, no allocation, no host synchronisation.
 * sos_silence_label_workspace_bytes: 256-byte-aligned int32 arrays of sum(frames) and sum(frames) + nclips entries; -1 on
 *   a null table or nclips outside 1 .. 65535.
 * SOS_EINVAL (sos_last_error() names the clip), before any launch: null pointers, nclips outside 1 .. 65535, a clip without
 * samples or frames, an entry outside the samples / frames summed from the host table, ratio <= 1, a minimum run length < 1, a
 * negative rel or floor, a frame count under which the last frame would be empty or samples would be left over; SOS_ENOSPC: a
 * workspace smaller than sos_silence_label_workspace_bytes says. */
int64_t sos_silence_label_workspace_bytes(const int64_t* table_host, int nclips);
int sos_silence_label_batch(const float* x, const int64_t* table, const int64_t* table_host, int nclips, const double* params,
                            const double* params_host, void* workspace, int64_t workspace_bytes, uint8_t* bits, double* energy,
                            double* out, sos_stream_t stream);

/* ---- noisy speech out of clean speech for a ragged batch of clips (csrc/ragged_mix.hip; sos_amd.tools.add_signals_ragged;
 * float64 restatement: tests/mix_reference.py): add_signals with one noise (M2/tools.py:217-276) around the silencing and the
 * zero-filled noise crop of the hand-off.  clips = the clips back to back in one f32 buffer.  table / table_host: int64
 * [nclips][4] on the device / the HOST, the rows of sos_ragged_stage_f32 {sample offset, samples, frame offset, frames}.
 * noise: f32 buffer of noise_total samples; noise_table / noise_table_host: int64 [nclips][2] = {noff, nz}: clip b is mixed with
 * noise[noff .. noff + nz), zero from nz to the clip's end (nz <= samples; nz = 0: a silent noise).  Crops of different clips may
 * overlap or coincide.  params / params_host: f64 [nclips][2] = {snr in dB, ratio = samples per frame (> 1), or 0 = the clip has
 * no frame decisions}; bits: the frame decisions back to back at the frame offsets (1 = non-silent), NULL if every ratio is 0.
 *   s = clip * (1 - mask) under the mask rule of sos_bits_to_mask (csrc/mask_rule.h), or the clip itself at ratio 0;
 *   Es = sum s^2, Ez = sum z^2 in f64; gain = 1 if Es == 0 or Ez == 0, else sqrt(Es / 10^(snr / 10)) / sqrt(Ez);
 *   m = s + gain z; peak = max |m|; inv = norm / peak if norm != 0 and peak != 0, else 1;
 *   mixed = m inv, clean = s inv, noise_out = gain z inv: f32, each back to back at the clips' sample offsets (sum(samples)
 *   floats each; they must not overlap `clips`).
 * out: f64 [nclips][6] = {Es, Ez, gain, peak, inv, status}; gain and inv are applied as f32 factors and reported as those f32
 * values.  A clip's outputs and its row have the same bits alone, in any batch, at any offset and in any order: sums and maxima
 * over chunks of SOS_MIX_CHUNK samples counted from the clip's first sample, fixed trees, no atomics.  status = -1: the DEVICE
 * tables or parameters leave what the host's sized (the bounds rule of the other ragged kernels); nothing is read or written for
 * that clip but its row.  Four launches whatever the number of clips, no allocation, no host synchronisation.
 * sos_ragged_mix_workspace_bytes: 256-byte-aligned arrays of nclips int64 and 3 f64 per chunk; -1 on a null table or nclips
 *   outside 1 .. 65535.
 * SOS_EINVAL (sos_last_error() names the clip), before any launch: null pointers, nclips outside 1 .. 65535, a clip without
 * samples, more than 2^40 samples in all, an entry outside the samples / frames summed from the host table, a non-finite snr or
 * norm, a ratio that is neither 0 nor > 1, a ratio without bits, a crop outside [0, noise_total) or longer than its clip;
 * SOS_ENOSPC: a workspace smaller than sos_ragged_mix_workspace_bytes says. */
#define SOS_MIX_CHUNK 4096
int64_t sos_ragged_mix_workspace_bytes(const int64_t* table_host, int nclips);
int sos_ragged_mix_f32(const float* clips, const int64_t* table, const int64_t* table_host, int nclips, const float* noise,
                       int64_t noise_total, const int64_t* noise_table, const int64_t* noise_table_host, const uint8_t* bits,
                       const double* params, const double* params_host, double norm, void* workspace, int64_t workspace_bytes,
                       float* mixed, float* clean, float* noise_out, double* out, sos_stream_t stream);

/* ---- long recordings as ragged batches of overlapping windows (csrc/ragged_window.hip; sos_amd.pipeline.denoise_long; float64
 * restatement of the plan and the stitch: tests/window_reference.py).  One launch each, whatever the number of windows; no
 * allocation, no host synchronisation.  table / table_host: int64 [nwin][10] on the device / the HOST, the rows of
 * pipeline.window_plan: {recording, source offset, samples, output offset, core start, core end, window start, row, previous
 * window, next window}.  Core start, core end and window start count samples of the window's own recording; the output offset
 * is where the window's first output sample lies in `out`; previous / next are table indices of the neighbouring windows of the
 * same recording, -1 at its ends.
 * sos_window_stage_f32: x holds `total` floats; rows [nwin][stride]: rows[w][0 .. samples) = x[source offset ..), zero from
 *   there to the stride.  Windows may overlap and may start on any sample.  Reads only {source offset, samples}, so one table
 *   stages several buffers through different source offsets.
 * sos_window_stitch_f32: rows f32 [n_rows][stride], window w in row `row`, its sample i being sample window start + i of its
 *   recording; out holds the recordings' outputs back to back, sum(core end - core start) floats: the cores must tile them.
 *   Window w is the one writer of its core.  A sample p of it that lies within `context` samples of a core boundary b shared
 *   with a neighbour is blended over the zone [b - context, b + context): w = (p - (b - context) + 0.5) / (2 context),
 *   out = (1 - w) earlier window + w later window, in f32; every other sample is copied bit for bit; context = 0 is a plain
 *   cut.  No atomics, fixed arithmetic: a recording's output has the same bits alone, in any batch, at any offset and with the
 *   table in any order.
 * SOS_EINVAL (sos_last_error() names the window), before any launch: null pointers, nwin outside 1 .. 65535, stride < 1,
 * samples > stride, a row outside n_rows, context < 0 or above 2^22, a context not less than a window it blends or more than
 * the core holds (twice with two neighbours), a core outside its window, a neighbour that is no window of the same recording
 * or does not cover the overlap, an entry outside `total` or outside the summed output length.  The kernels follow the DEVICE
 * table and skip an entry that fails the same tests. */
int sos_window_stage_f32(const float* x, int64_t total, const int64_t* table, const int64_t* table_host, int nwin, int64_t stride,
                         float* rows, sos_stream_t stream);
int sos_window_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table, const int64_t* table_host,
                          int nwin, int64_t context, float* out, sos_stream_t stream);

/* ---- several signals of the same plan stitched in ONE launch, written where a download wants them (csrc/ragged_window.hip;
 * the four signals of sos_amd.pipeline.denoise_long(signals=True) and of the windowed hand-off).
 * sos_window_stitch_planes_f32: rows f32 [planes][n_rows][stride], planes 1 .. 8: plane q of window w is row q * n_rows + row.
 *   table / table_host: the plan table above, unchanged; column 0 (the recording) is read here, to find the destination, and
 *   column 3 is validated exactly as sos_window_stitch_f32 validates it, so one plan serves both calls.  recs / recs_host:
 *   int64 [nrec][2] = {base, pitch}: sample p of plane q of recording r -- p counts within the recording's own output,
 *   0 .. len_r, len_r = the sum of its cores -- goes to out[base_r + q * pitch_r + p]; out holds out_total floats.
 *   base = the recording's output offset and pitch = out_total / planes is the plane-major layout [planes][sum len]; base = where
 *   the recording's block starts and pitch >= len_r puts the planes of one recording next to each other (file-major).
 *   pitch > len_r leaves a gap that is never written (it keeps a segment's start a multiple of four floats: 16-byte stores).
 *   Each plane holds, bit for bit, what sos_window_stitch_f32 writes for that plane alone: the same one-writer-per-core rule,
 *   weights and blend (one __device__ function serves both kernels); no atomics; a result does not depend on the batch, the
 *   table order, the row order or the destination's alignment.
 * SOS_EINVAL (sos_last_error() names the window or the recording), before any launch: everything sos_window_stitch_f32
 * refuses, planes outside 1 .. 8, nrec outside 1 .. 65535, out_total < 0, a window whose recording is outside nrec or whose core
 * ends past its recording's len_r, neighbours of different recordings, pitch < len_r, a (recording, plane) segment outside
 * out_total, two segments that overlap.  The kernel follows the DEVICE tables and skips a window that fails the same tests. */
int sos_window_stitch_planes_f32(const float* rows, int planes, int64_t n_rows, int64_t stride, const int64_t* table,
                                 const int64_t* table_host, int nwin, int64_t context, const int64_t* recs,
                                 const int64_t* recs_host, int nrec, int64_t out_total, float* out, sos_stream_t stream);

/* ---- one decision stream per recording, and windows masked by it (csrc/ragged_window.hip; sos_amd.pipeline.detect_long and the
 * `bits=` path of denoise_long; float64 restatement of the frame stitch: tests/frames_reference.py).  One launch each.
 * sos_window_frames_stitch_f32: rows f32 [n_rows][stride] hold the windows' frame logits, window w (an entry of the plan table
 *   above, of which {core start, core end, window start, row} are read) in row `row` with frames[w] logits (frames /
 *   frames_host: int64 [nwin], 1 .. stride).  recs / recs_host: int64 [nrec][4] = {frame offset in `out`, frames F, first
 *   window, windows K}: the windows first .. first + K - 1 of the table are the recording's, in order; ratios / ratios_host:
 *   f64 [nrec], rho = samples per frame, in (0, 2^30]; F <= 2^31.  out: the recordings' F logits each, sum(F) floats.  Frame i
 *   of a recording has the centre p = (i + 0.5) rho (float64, one rounded multiply) and the owner k = min(floor(p) / core,
 *   K - 1); window q gives for it its frame j_q = clamp(floor((i + 0.5) - start_q / rho), 0, frames_q - 1) (one rounded divide,
 *   one rounded subtract).  out[i] = rows[k][j_k], a bit-for-bit copy, except with context > 0 in the zones
 *     k > 0     and p <  core start_k + context: w = (p - (core start_k - context)) / (2 context), out = (1 - w) rows[k-1][j_{k-1}] + w rows[k][j_k]
 *     k < K - 1 and p >= core end_k - context:   w = (p - (core end_k - context)) / (2 context),   out = (1 - w) rows[k][j_k] + w rows[k+1][j_{k+1}]
 *   with w computed in float64, rounded once to f32, and the blend in f32.  core >= 2 context keeps the zones apart.  One
 *   writer per output frame, no atomics: the same bits alone, in any batch, at any offset, with the rows in any order.
 * sos_window_stage_masked_f32: x = the recordings back to back, bits = their frame decisions back to back (1 = non-silent),
 *   clips / clips_host + ratios / ratios_host: the recordings' table {sample offset, samples, bit offset, frames} and samples
 *   per frame (> 1) as sos_ragged_stage_f32 takes them; table / table_host: the plan table, of which {recording, source offset,
 *   samples, window start} are read (source offset = the recording's sample offset + window start).  wave, masked f32
 *   [nwin][stride]: wave[w][j] = x[source offset + j], masked[w][j] = wave[w][j] * mask, mask = the value sos_ragged_stage_f32 /
 *   sos_bits_to_mask give sample window start + j of the WHOLE recording (its frames, its ratio, its last sample for the
 *   short-run flip); both zero from the window's samples to the stride.  Rows equal slices of sos_ragged_stage_f32's
 *   full-length wave / masked bit for bit; nothing of full length is written.
 * SOS_EINVAL before any launch (sos_last_error() names the window or the recording): null pointers, nwin / nrec outside
 * 1 .. 65535, stride < 1, core < 1, context < 0 or above 2^22, core < 2 context, a recording outside the summed frames /
 * samples / the table's windows, a ratio outside its range, a window with a row outside n_rows, frames outside 1 .. stride,
 * samples > stride, or samples outside its recording.  The kernels follow the DEVICE tables and skip an entry that fails
 * the same tests. */
int sos_window_frames_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table, const int64_t* table_host,
                                 const int64_t* frames, const int64_t* frames_host, int nwin, const int64_t* recs,
                                 const int64_t* recs_host, const double* ratios, const double* ratios_host, int nrec, int64_t core,
                                 int64_t context, float* out, sos_stream_t stream);
int sos_window_stage_masked_f32(const float* x, const uint8_t* bits, const int64_t* clips, const int64_t* clips_host,
                                const double* ratios, const double* ratios_host, int nrec, const int64_t* table,
                                const int64_t* table_host, int nwin, int64_t stride, float* wave, float* masked,
                                sos_stream_t stream);

/* ---- one decision stream shared by the recordings of a group -- the channels of a file (csrc/ragged_window.hip;
 * sos_amd.windows.detect_long(link=); numpy restatement of the reduction and the decision: tests/link_reference.py).
 * sos_window_frames_link_f32 is sos_window_frames_stitch_f32 with a link table, in ONE launch: rows, table, frames, recs,
 *   ratios, core and context are that call's, and every member recording's frame i is stitched by that call's rule (one
 *   __device__ function serves both kernels: the same bits).  Column 0 of `recs`, a recording's own frame offset, is NOT used
 *   for output here and is not validated.  links / links_host: int64 [ngroups][4] = {frame offset of the group's stream in the
 *   outputs, frames F, first index into `members`, member count}; members / members_host: int64 recording indices (rows of
 *   `recs`), sum(member count) of them.  Frame i of group g is reduced over its members IN MEMBER ORDER --
 *     mode 0 (any):  x = fmaxf(... fmaxf(v_0, v_1) ..., v_last)          (bit 1 = non-silent: speech if any member has speech)
 *     mode 1 (mean): x = (((v_0 + v_1) + ...) + v_last) / (float)count   (f32 sum, one f32 divide)
 *   -- a group of one keeps its member's logits bit for bit in both modes -- and decided as sos_threshold_bits decides:
 *   out_logits[offset + i] = x, out_bits[offset + i] = 1 / (1 + expf(-x)) >= threshold (mask_rule.h, one statement for
 *   both).  out_logits f32 and out_bits uint8 hold sum(F) elements each, the groups' streams back to back.  One thread and
 *   one writer per output frame, no atomics, no LDS.  A recording that is in no group is not read.
 * SOS_EINVAL before any launch, without touching the device (sos_last_error() names the group, the member or the window): null
 * pointers, the argument rules of sos_window_frames_stitch_f32, ngroups outside 1 .. 65535, a mode other than 0 or 1, a
 * threshold that is not finite, a group without members or with more than nrec, member ranges outside the sum of the member
 * counts, a group stream outside sum(F) or overlapping another, a member index outside nrec, a recording that appears twice (in
 * two groups or in one), a member whose frames differ from its group's or whose ratio differs from the group's first member's,
 * and for every member what sos_window_frames_stitch_f32 refuses of a recording and its windows.  The kernel follows the
 * DEVICE tables and gives a group or a frame that fails the same tests no work. */
int sos_window_frames_link_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table, const int64_t* table_host,
                               const int64_t* frames, const int64_t* frames_host, int nwin, const int64_t* recs,
                               const int64_t* recs_host, const double* ratios, const double* ratios_host, int nrec, int64_t core,
                               int64_t context, const int64_t* links, const int64_t* links_host, const int64_t* members,
                               const int64_t* members_host, int ngroups, int mode, float threshold, float* out_logits,
                               uint8_t* out_bits, sos_stream_t stream);

/* ---- live audio denoised in windows, the state between two calls on the device (csrc/stream_window.hip;
 * sos_amd.pipeline.StreamDenoiser; the rule: pipeline.StreamPlan, float64 restatement tests/stream_reference.py).  One launch
 * each whatever the number of slots; no allocation, no host synchronisation, no atomics.  A slot is one stream.
 *   ring f32 [slots][cap]: sample p of the stream of slot s lies at ring[s][p % cap].
 *   tail f32 [slots][2][2 context]: the overlap [b - context, b + context) of the last window's row around its core end b.
 * Every table comes twice, on the device and on the HOST (int64 rows).
 * sos_stream_push_f32: flat holds `total` floats, the chunks back to back; rows {slot, source offset, samples, stream position}:
 *   ring[slot][(position + j) % cap] = flat[source offset + j], j < samples.  samples <= cap (0: nothing is written); a slot
 *   appears at most once per table.
 * sos_stream_stage_f32: rows {slot, stream position, samples}; rows f32 [nwin][stride]: rows[w][j] = ring[slot][(position + j)
 *   % cap] for j < samples, zero from there to the stride (sos_window_stage_f32 with a modular source index).  samples <= cap
 *   and <= stride.
 * sos_stream_stitch_f32: rows f32 [n_rows][stride]; table rows {slot, row, window start, samples of the row, core start, core
 *   end, flags, parity}: sample i of row `row` is sample window start + i of the stream; flags: 1 = a window ran before this
 *   one, 2 = one will run after it.  out f32 [nwin][out_stride]: out[w][0 ..] = the samples [lo, hi) of the stream that are
 *   final after this window, lo = core start - context with a previous window (else core start), hi = core end - context with
 *   a next one (else core end).  With a previous window the first 2 context of them are blended with tail[slot][parity]:
 *   w = (i + 0.5) / (2 context), out = (1 - w) tail + w row, in f32 -- the statement and the bits of sos_window_stitch_f32;
 *   every other sample is copied bit for bit.  With a next window the row's samples [core end - context, core end + context)
 *   go to tail[slot][parity ^ 1]: the caller flips the slot's parity after such a call.  context = 0 is a plain cut.  The
 *   grid follows nwin, the strides and the context alone; a slot's bits do not depend on the other rows, its slot index or the
 *   table's order.
 * SOS_EINVAL before any launch (sos_last_error() names the row): null pointers, rows or slots outside 1 .. 65535, cap or a
 * stride < 1, a slot outside the slots, a slot twice in one table (push, stitch), samples above cap or the stride, a negative
 * position, a chunk outside `total`, a row outside n_rows, a core outside its row, an overlap outside its row, more context
 * than the core holds, flags outside 0 .. 3, a parity outside 0 .. 1, more emitted samples than out_stride, context < 0 or
 * above 2^22.  The kernels follow the DEVICE table and skip a row that fails the same bounds. */
int sos_stream_push_f32(const float* flat, int64_t total, const int64_t* table, const int64_t* table_host, int nrows, float* ring,
                        int64_t slots, int64_t cap, sos_stream_t stream);
int sos_stream_stage_f32(const float* ring, int64_t slots, int64_t cap, const int64_t* table, const int64_t* table_host, int nwin,
                         int64_t stride, float* rows, sos_stream_t stream);
int sos_stream_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table, const int64_t* table_host,
                          int nwin, int64_t slots, int64_t context, float* tail, float* out, int64_t out_stride,
                          sos_stream_t stream);

/* ---- live audio resampled in chunks, the state between two calls on the device (csrc/stream_resample.hip;
 * sos_amd.audio_io.StreamResampler; float64 restatement of the rule: tests/stream_resample_reference.py).  Notation of
 * sos_resample_f32: scale = min(1, ratio), index_step = (int)(scale * num_table), time(t) = resampy's running f64 sum,
 * n(t) = floor(time(t)); R = nwin / index_step bounds what either wing of an output reads.
 * sos_stream_resample_ready (host only, no HIP call): after n_recv samples of a stream, *t_ready = the number of outputs that are
 *   final -- every t with n(t) + 1 + R <= n_recv: computed with n_in = n_recv it has the value it has for any longer signal --
 *   and *base = max(n(t_ready) - (R - 1), 0), the first sample a later output still reads.  n_recv - *base <= 2 R - 1.  Both
 *   come from the running sum the kernel evaluates.  SOS_EINVAL: ratio <= 0, nwin < 1, num_table < 1, index_step < 1,
 *   n_recv < 0 or above 2^52, null pointers; SOS_ENOSPC: the time register needs more segments than the kernel argument holds.
 * sos_stream_resample_f32: ONE launch whatever nrows is.  ring f32 [slots][cap] as sos_stream_push_f32 writes it (sample p of
 *   the stream of slot s at ring[s][p % cap]); win, nwin, num_table: as sos_resample_f32.  table: int64 [nrows][6] on the device,
 *   table_host: the same values on the HOST; a row is
 *     {slot, t_lo, t_hi, n_in, n_valid, output offset}
 *   and writes the outputs t_lo <= t < t_hi of the slot's stream to out[output offset ..] (out holds `total` floats): output t
 *   as sos_resample_f32 computes it for a signal of n_in samples, zero for t >= n_valid.  While a stream runs, n_in = the
 *   samples received, t_hi <= *t_ready and n_valid = t_hi; at its end n_in = its length, n_valid = (int64)(n_in * ratio) and
 *   t_hi = the output length.  The concatenated outputs of a stream are bit for bit what sos_resample_f32 writes for the whole
 *   signal, whatever the chunking, the slot, the other rows and the table's order.  The time register starts at 0 for every
 *   stream and is built up to the largest t_hi of the call; if it needed more segments than the kernel argument holds (120)
 *   that would be SOS_ENOSPC before the launch.  It does not within the positions accepted: it takes about two segments per
 *   binade of the register, 102 for the 2^52 input samples of a 48 -> 14 kHz stream (counted on the host with
 *   sos_resample_time_segments), so the bound on a stream is n_in <= 2^52: 2 970 years at 48 kHz.
 * SOS_EINVAL before any launch (sos_last_error() names the row): null pointers, rows or slots outside 1 .. 65535, cap < 1, a
 * slot outside the slots, a slot twice in one table, t_lo < 0 or t_lo > t_hi, n_in < 0, n_valid outside 0 .. (int64)(n_in * ratio),
 * output offset + (t_hi - t_lo) > total, a row that reads a sample at or past n_in or more than `cap` samples before n_in (its
 * ring does not hold them any more), the filter refusals above, (nwin + 1) * 4 bytes > 160 KB.  The kernel follows the DEVICE
 * table and skips a row that fails the same bounds. */
int sos_stream_resample_ready(double ratio, int nwin, int num_table, int64_t n_recv, int64_t* t_ready, int64_t* base);
int sos_stream_resample_f32(const float* ring, int64_t slots, int64_t cap, const int64_t* table, const int64_t* table_host, int nrows,
                            double ratio, const float* win, int nwin, int num_table, float* out, int64_t total, sos_stream_t stream);

/* ---- the band above the networks' half rate for LIVE audio (csrc/stream_band.hip; sos_amd.audio_io.StreamBandMerger; float64 /
 * integer restatement of the rule: tests/stream_band_reference.py).  The rule of sos_resample_merge_batch_f32 for streams that
 * arrive in chunks, with its bits: x = the native stream, a = x at the low rate, b = the networks' output, U = the resampling
 * back at ratio = native rate / low rate > 1 (an upsampling: scale = 1, index_step = num_table, R = nwin / num_table),
 *     out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t]).
 * State on the device: ring f32 [3 slots][cap] as sos_stream_push_f32 writes it -- row slot holds x, row slots + slot holds a,
 * row 2 slots + slot holds b of the stream of `slot`, sample p at [p % cap] -- and rring f64 [slots][rcap], frame j of r at
 * [j % rcap].  smooth = K, the frames of smoothing on each side (0 .. 16); smooth < 0: no gains, g = 1 ('keep').
 * The rule.  With n_x native samples and m_b samples of b received (a is never behind b) output t is final -- it has the bits
 * it has for any longer stream -- once (1) n(t) + 1 + R <= m_b: neither right wing is cut, sos_stream_resample_ready asked
 * about m_b; (2) with gains, F(t) < m_b / hop - K, where p = (t + 0.5) / (ratio hop) - 0.5 in f64 and F(t) = 0 for p <= 0,
 * floor(p) + 1 otherwise, is the last frame of s that g[t] reads: r[j] is final once (j + 1) hop <= m_b, s[j] once r[j + K] is,
 * and then neither the clamp at J - 1 nor the cut of the mean at the clip's end can reach it; (3) t < n_x.
 * sos_stream_band_ready (host only, no HIP call): *t_ready = T, the number of final outputs (they are a prefix); what later
 *   outputs still read: x from *first_x = T, a and b from *first_a = *first_b = max(n(T) - (R - 1), 0), with gains also no
 *   later than hop (m_b / hop), the first sample of a frame without r; r from *first_r = max(F(T) - 1 - K, 0).  All from the
 *   expressions the kernels evaluate.  SOS_EINVAL: ratio <= 1, a wing below one sample, hop outside 1 .. 2^20, smooth > 16,
 *   counts negative or above 2^52, null pointers; SOS_ENOSPC as sos_stream_resample_ready.
 * sos_stream_band_ratio_f64: ONE launch whatever nrows is; table int64 [nrows][5], a row is {slot, j_lo, j_hi, m_a, m_b}:
 *   r[j] for j_lo <= j < j_hi into the slot's ring of frames, frame j covering the samples [j hop, (j + 1) hop) cut at m_a, b
 *   reading zero from m_b on: sos_band_gain_batch_f32's r, bit for bit.  While a stream runs j_hi = m_b / hop; at its end m_a =
 *   m, m_b = m' and j_hi = J = ceil(m / hop), which gives the last partial frame the file path's r.
 * sos_stream_band_merge_f32: ONE launch whatever nrows is; table int64 [nrows][10], a row is
 *     {slot, t_lo, t_hi, n_x, n_a, n_b, v_b, J, r_hi, output offset}
 *   and writes the outputs t_lo <= t < t_hi of the slot's stream to out[output offset ..] (out holds `total` floats), computed as
 *   of n_x native samples, signals a of n_a and b of n_b samples (U(b) zero from output v_b on), r_hi frames of r written so
 *   far, and J frames of s -- J = -1 while the stream is open: no end is known, none clamps.  While a stream runs t_hi <= T,
 *   v_b = t_hi; at its end n_a = m, n_b = m', v_b = (int64)(m' * ratio), J = r_hi = ceil(m / hop), t_hi = n.  s is formed per
 *   output from r (the two means, then the interpolation) with sos_band_gain_batch_f32's and sos_resample_merge_batch_f32's
 *   expressions.  The concatenated outputs of a stream are bit for bit what sos_resample_merge_batch_f32 writes for the whole
 *   signals, whatever the chunking, the slot, the other rows and the table's order.
 * SOS_EINVAL before any launch (sos_last_error() names the row): null pointers (rring may be null without gains), rows outside
 * 1 .. 65535, slots outside 1 .. 21845, cap or rcap < 1, a slot outside the slots or twice in one table, ranges that are none,
 * n_b > n_a, v_b above (int64)(n_b * ratio), output offset + (t_hi - t_lo) > total, a row that reads x at or past n_x or more
 * than `cap` before it, a or b at or past their counts or more than `cap` before n_a, frames of r at or past r_hi or more than
 * `rcap` before it, frames of a beyond ceil(m_a / hop), with an end J other than ceil(n_a / hop) or than r_hi, the filter
 * refusals above, (nwin + 1) * 4 bytes > 160 KB.  The kernels follow the DEVICE table and skip a row that fails the same
 * bounds; every ring index is modular. */
int sos_stream_band_ready(double ratio, int nwin, int num_table, int hop, int smooth, int64_t m_b, int64_t n_x, int64_t* t_ready,
                          int64_t* first_x, int64_t* first_a, int64_t* first_b, int64_t* first_r);
int sos_stream_band_ratio_f64(const float* ring, int64_t slots, int64_t cap, const int64_t* table, const int64_t* table_host,
                              int nrows, int hop, double* rring, int64_t rcap, sos_stream_t stream);
int sos_stream_band_merge_f32(const float* ring, int64_t slots, int64_t cap, const double* rring, int64_t rcap, const int64_t* table,
                              const int64_t* table_host, int nrows, double ratio, const float* win, int nwin, int num_table, int hop,
                              int smooth, float* out, int64_t total, sos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SOS_HIP_H */
