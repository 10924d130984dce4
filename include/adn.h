/*
 * adn.h — C ABI of libadn.so, the MI355X (gfx950) implementation of the AudioDenoiser hot path.
 *
 * The reference (jimonld2000/AudioDenoiser) is pure Python and has no FFI of its own; its boundary for this
 * path is the Python API of code/model.py, code/data_loader.py and the two STFT helpers.  Each entry point
 * below replaces the arithmetic behind one of those Python call sites (cited per function); the Python
 * mirror in audiodenoiser_amd/{model,stft,data_loader}.py binds them with ctypes (see INTEGRATION.md for the
 * stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C types only: device pointers are raw `float*`, the stream is a `hipStream_t` passed as `void*`
 *     (NULL = the null stream).  No torch / C++ types cross this boundary.
 *   - every function returns an int status (ADN_OK = 0); on failure adn_last_error() returns a thread-local
 *     message.  Nothing throws or aborts across the ABI.
 *   - work is enqueued on the caller's stream.  The only calls that block or allocate: adn_unet_create / adn_unet_destroy
 *     (one-time weight upload / free), adn_prepare, and the FIRST call per (device, n_fft) of an STFT-family entry point
 *     (adn_stft_mag, adn_stft_mag_fit, adn_stft_complex, adn_istft, adn_griffin_lim, adn_denoise_resynth, adn_stream_analyze, adn_stream_emit, adn_stream_pool_analyze, adn_stream_pool_emit) or per device of adn_perceptual_loss / adn_perceptual_loss_backward, which
 *     builds a few KB of constant tables (window, twiddles, mel filters) with a blocking upload -- unless adn_prepare did so
 *     before; and the FIRST adn_resample or adn_resample_stream per (device, rate pair), which builds its coefficient table
 *     (adn_resample_prepare builds both).  Such a cold call on a stream that is being captured enqueues nothing and returns ADN_ERR_INVALID (never a HIP
 *     error): call adn_prepare(device, n_fft) before capturing.  adn_unet_forward never blocks or allocates.
 *   - ownership: the caller owns every buffer it passes (x, y, audio, out, workspace); a handle owns only
 *     its packed (BatchNorm-folded, re-laid-out) weights.
 *   - a handle is bound to one device and is not re-entrant: one forward at a time per handle.  Entry points that
 *     take a handle run on the handle's device and restore the caller's current device before returning; the
 *     handle-free entry points (STFT, loader, losses, Griffin-Lim) run on the caller's current device.
 *   - alignment: workspaces 16 bytes; complex spectrograms (float pairs) 8 bytes; everything else 4 bytes
 *     (ADN_ERR_INVALID otherwise).  Any hipMalloc / PyTorch allocation satisfies this.
 *   - there is NO CPU implementation in this library.
 */
#ifndef ADN_H
#define ADN_H

#include <stddef.h>

/* The 80 functions below are the ONLY symbols libadn.so exports: the library is built with -fvisibility=hidden and linked with
 * a version script (audiodenoiser_amd/csrc/libadn.map: `adn_*` global, everything else local). */
#if defined(__GNUC__)
#define ADN_API __attribute__((visibility("default")))
#else
#define ADN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ADN_OK 0
#define ADN_ERR_INVALID 1      /* bad argument (shape, null pointer, unsupported size) */
#define ADN_ERR_HIP 2          /* a HIP runtime call failed; message carries hipGetErrorString */
#define ADN_ERR_WORKSPACE 3    /* workspace too small */
#define ADN_ERR_NO_DEVICE 4    /* no gfx950 device visible */

#define ADN_N_WEIGHT_TENSORS 118   /* state_dict float tensors (136 entries minus 18 num_batches_tracked) */
#define ADN_N_TAPS 10              /* down1..down4, bottleneck, up1..up4, out */
#define ADN_N_LAUNCHES 23          /* timing slots per forward: first conv, 17 MFMA 3x3 convs, 4 convT, 1x1 out; a slot
                                      whose layer runs fused into its neighbour (1x1 out: only the tail that adds the
                                      partial planes remains; first conv on the F(2x2,3x3) path) stays ~0 */

typedef struct adn_unet adn_unet;

/* Library / diagnostics --------------------------------------------------------------------------------- */
ADN_API int adn_version(void);
ADN_API const char *adn_last_error(void);
ADN_API int adn_device_count(int *count);
/* Builds the constant tables the handle-free entry points need on `device`: the window / twiddle tables of `n_fft` (a power
 * of two in [64, 4096]; 0 = none) and the mel filterbank of adn_perceptual_loss.  Synchronous (blocking upload), idempotent,
 * thread-safe.  After it, every adn_stft_* / adn_istft / adn_griffin_lim call with that n_fft and adn_perceptual_loss only
 * enqueue on the caller's stream, so they can be captured into a HIP graph (e.g. adn_stft_mag_fit + adn_unet_forward, the
 * wav -> network path of the reference's test.py:94-113). */
ADN_API int adn_prepare(int device, int n_fft);

/* U-Net forward: replaces UNet.forward (reference code/model.py:70-94) and everything it calls —
 * DoubleConvLayer (model.py:7-20), DownSampleLayer (model.py:23-32), UpSampleLayer (model.py:35-50). ----- */

/* Build a handle from the 118 fp32 HOST tensors of `UNet(1,1).state_dict()` in state_dict order with the
 * num_batches_tracked entries skipped (per conv+BN pair: conv.weight, conv.bias, bn.weight, bn.bias,
 * bn.running_mean, bn.running_var; per UpSampleLayer first up.weight, up.bias; finally out.weight, out.bias).
 * This is the weight format of the reference checkpoint (train.py:142, test.py:65).  BatchNorm (eval mode,
 * eps 1e-5) is folded into the preceding convolution here.  Synchronous. */
ADN_API int adn_unet_create(adn_unet **handle, int device, const float *const *host_tensors, int n_tensors);
/* Same with an explicit arithmetic type.  ADN_DTYPE_F32 (= adn_unet_create): exact-fp32 matrix cores.
 * ADN_DTYPE_F16 (BASELINE configs[4]): activations and weights stored in fp16 inside the library, fp16 MFMA
 * with fp32 accumulation; x and y stay fp32 at the boundary; outputs within 1e-2 of the fp32 path. */
#define ADN_DTYPE_F32 0
#define ADN_DTYPE_F16 1
ADN_API int adn_unet_create_ex(adn_unet **handle, int device, const float *const *host_tensors, int n_tensors, int dtype);
/* UNet(in_channels, num_classes) as the reference declares it (code/model.py:54,56,68; its own callers use (1, 1), test.py:63):
 * the same 118 tensors with downconv1.conv.double_conv.0.weight (64, in_channels, 3, 3), out.weight (num_classes, 64, 1, 1) and
 * out.bias (num_classes).  x is then (N, in_channels, F, T) and y (N, num_classes, F, T), both NCHW fp32.  1 <= in_channels <= 64,
 * 1 <= num_classes <= 64.  With more than one input plane / class the first / last
 * convolution run as their own launches (the fused forms are for one plane / one class). */
ADN_API int adn_unet_create_general(adn_unet **handle, int device, const float *const *host_tensors, int n_tensors, int dtype,
                            int in_channels, int num_classes);
ADN_API int adn_unet_channels(const adn_unet *handle, int *in_channels, int *num_classes);
/* Kernel choice by the launch's grid.  Default (on = 0): fp32 3x3 layers run F(4x4,3x3) where its 32x32-pixel tiles fill the chip,
 * F(2x2,3x3) otherwise; layers whose grid is still too small (one clip ... a dozen, at the deep levels) have their K loop cut over
 * up to 8 workgroups + a reduce launch -- fp32 3x3 layers (either Winograd form), fp32 transposed convolutions, fp16 3x3 layers.  Fastest at every batch
 * size, but the same clip computed alone and inside a large batch then differs in the last bits (fp32: both within 1e-4 of the
 * reference; fp16: within 5e-3 of each other, both within 1e-2 of the reference).
 * on = 1: one kernel per layer chosen by the layer's geometry alone -- a clip's result is bit-identical whatever batch it is
 * computed in (evaluation / regression runs that compare across batch sizes), fp32 and fp16 handles alike.  May be changed
 * between forwards.  Initial value: 0, or the environment's ADN_BATCH_INVARIANT when the handle is created. */
ADN_API int adn_unet_set_batch_invariant(adn_unet *handle, int on);
ADN_API int adn_unet_destroy(adn_unet *handle);

/* Bytes of device scratch adn_unet_forward needs for an (N,1,F,T) batch (half as much for an fp16 handle;
 * handle may be NULL = fp32). */
ADN_API int adn_unet_workspace_bytes(const adn_unet *handle, int N, int F, int T, size_t *bytes);

/* y(N,K,F,T) = UNet(x(N,C,F,T)) (C = K = 1 unless the handle came from adn_unet_create_general), eval-mode semantics
 * (BatchNorm uses running statistics), fp32.
 * x, y, workspace: device memory on the handle's device.  F,T >= 16 (four 2x poolings). */
/* Shape limits: N >= 1, F >= 16, T >= 16, F*T < 2^27 (ADN_ERR_INVALID otherwise) -- e.g. 513 bins x 261 000 frames; the workspace
 * (adn_unet_workspace_bytes: ~1.1 KB per pixel in fp32, half in fp16) is the practical bound. */
ADN_API int adn_unet_forward(adn_unet *handle, const float *x, float *y, int N, int F, int T,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Same, additionally exporting block outputs as NCHW fp32 device tensors for parity tests: taps[i] may be
 * NULL (skipped) or a buffer of the block's size, i = 0..3 skip tensors down1..4 (DownSampleLayer's first
 * return value), 4 bottleneck, 5..8 up1..4, 9 out. */
ADN_API int adn_unet_forward_taps(adn_unet *handle, const float *x, float *y, int N, int F, int T,
                          void *workspace, size_t workspace_bytes, float *const *taps, void *stream);

/* Measurement hook (bench.py's roofline object): with timing enabled every kernel launch of adn_unet_forward
 * is bracketed by hipEventRecord on the caller's stream (events are created here, never in the forward).
 * max_forwards = 0 disables.  adn_unet_get_timing synchronises on the events of forward number `index`
 * (0-based since the last adn_unet_set_timing) and returns the ADN_N_LAUNCHES kernel durations in
 * milliseconds, in launch order: conv_first; conv3x3+pool (down1); [conv3x3, conv3x3+pool] x3 (down2..4);
 * conv3x3 x2 (bottleneck); [convT, conv3x3(cat), conv3x3] x4 (up1..4); conv1x1 out. */
ADN_API int adn_unet_set_timing(adn_unet *handle, int max_forwards);
ADN_API int adn_unet_get_timing(adn_unet *handle, int index, float *ms);

/* STFT magnitude: replaces audio_to_magnitude_spectrogram (code/create_train_dataset.py:162-174,
 * center=0) and audio_to_spectrogram (code/create_test_dataset.py:35-41, center=1), i.e.
 * librosa.stft(y, n_fft, hop_length, center, window="hann", pad_mode="constant") + librosa.magphase. ------- */
ADN_API int adn_stft_n_frames(long length, int n_fft, int hop, int center, long *n_frames);
/* audio (n_clips, length) fp32 -> out (n_clips, n_fft/2+1, n_frames) fp32, frame index fastest.
 * n_fft: power of two in [64, 4096]; hop >= 1. */
ADN_API int adn_stft_mag(const float *audio, int n_clips, long length, int n_fft, int hop, int center,
                 float *out, void *stream);

/* STFT magnitude fused with the loader rule that follows it on the wav -> network path: out (n_clips, H, W) =
 * fp32(fp16(|STFT|)) cropped / zero padded at the bottom and right to (H, W), i.e. adn_quantize_pad(adn_stft_mag(...))
 * (code/data_loader.py:41-42,54-72 applied to code/create_test_dataset.py:35-41) in one kernel: only the min(n_frames, W)
 * frames inside the window are computed, nothing is written outside it, rows are W floats apart.  Bit-identical to the
 * two-step form. */
ADN_API int adn_stft_mag_fit(const float *audio, int n_clips, long length, int n_fft, int hop, int center,
                     float *out, int H, int W, void *stream);

/* Loader arithmetic: replaces SpectrogramDataset.__getitem__/_pad_or_truncate (code/data_loader.py:41-42,
 * 54-72) for a batch already on the device: out(n,H,W) = fp32(fp16(in(n,h,w))) cropped / zero padded at the
 * bottom and right. */
ADN_API int adn_quantize_pad(const float *in, int n, int h, int w, float *out, int H, int W, void *stream);

/* Per-clip mean absolute error, the payload of the multi-GPU all-gather (F.l1_loss per clip, cf.
 * code/loss.py:86):  out[i] = mean_j |a[i,j] - b[i,j]|. */
ADN_API int adn_per_clip_l1(const float *a, const float *b, int n_clips, long elems_per_clip, float *out, void *stream);

/* Per-clip CombinedPerceptualLoss: replaces, clip by clip, CombinedPerceptualLoss.forward and the two losses it
 * calls (code/loss.py:6-95; caller code/test.py:118-122).  pred, target: (n_clips,1,F,T) fp32 device tensors;
 * out: (n_clips,4) = {total, stft, mel, l1}.  The reference's batch values are the means over clips (equal clip
 * sizes).  Constants are the reference's: scales (63,16),(32,8),(16,4); mel: sr 8000, n_fft 63, hop 16, 64 mels;
 * weights 0.4/0.4/0.2.  Needs T >= 32 (the mel term's reflect padding; the reference raises below that too) and
 * adn_perceptual_loss_workspace_bytes of device scratch.  Up to 6784 frames a clip's frequency-mean series and mel spectra are held
 * in the LDS of one CU; longer clips (no limit in the reference) keep the series in the workspace and walk the mel frames in blocks. */
ADN_API int adn_perceptual_loss_workspace_bytes(int n_clips, int F, int T, size_t *bytes);
ADN_API int adn_perceptual_loss(const float *pred, const float *target, int n_clips, int F, int T, void *workspace,
                        size_t workspace_bytes, float *out, void *stream);
/* Backward of adn_perceptual_loss (what loss.backward() needs in the reference's train.py:67-68): the exact chain rule of
 * the four per-clip outputs with respect to both inputs, as torch autograd differentiates the reference's loss (abs'(0) = 0,
 * sign(0) = 0; zero-padded STFT samples drop out, reflected mel samples fold back onto the series).
 * grad_out: device (n_clips, 4) fp32, d(objective)/d{total, stft, mel, l1} per clip.
 * grad_pred, grad_target: device (n_clips, 1, F, T) fp32, written (not accumulated); either may be NULL, not both.
 * Same shape limits as adn_perceptual_loss (T >= 32); adn_perceptual_loss_backward_workspace_bytes of device scratch (16-byte
 * aligned).  The mel filterbank is the one adn_perceptual_loss / adn_prepare builds.  Deterministic: no float atomics, two calls
 * give bit-identical gradients. */
ADN_API int adn_perceptual_loss_backward_workspace_bytes(int n_clips, int F, int T, size_t *bytes);
ADN_API int adn_perceptual_loss_backward(const float *pred, const float *target, int n_clips, int F, int T,
                                         const float *grad_out, void *workspace, size_t workspace_bytes,
                                         float *grad_pred, float *grad_target, void *stream);

/* ---- resampling and SNR noise mixing: the ingest of the training path --------------------------------------------------------
 * adn_resample replaces the rate conversion of librosa.load(path, sr=SAMPLE_RATE) (code/create_train_dataset.py:204,217,
 * code/create_test_dataset.py:144).  librosa resamples with soxr; this library DEFINES its own filter instead (soxr's taps are
 * not reproduced: parity with librosa.load is unpinned, like the STFT's parity with librosa), chosen so that an independent
 * implementation exists -- with the taps h below, scipy.signal.resample_poly(x, up, down, window=h / up) is the same operator.
 *   g = gcd(src_rate, dst_rate), up = dst_rate / g, down = src_rate / g, q = max(up, down)
 *   prototype low-pass on the up-times oversampled grid, length 2*half + 1, half = ZEROS * q:
 *     h[j] = up * fc * sinc(fc * j) * kaiser(2*half + 1, BETA)[j + half],  j = -half .. half,  fc = ROLLOFF / q,
 *     sinc(t) = sin(pi t) / (pi t), kaiser = numpy.kaiser;  ZEROS = 32, BETA = 12.0, ROLLOFF = 0.88
 *   output length M = ceil(L * up / down) (adn_resample_length; librosa's and scipy's rule)
 *   y[m] = sum_i x[i] * h[m*down - i*up] over the i with |m*down - i*up| <= half and 0 <= i < L
 *     (zero extension at both ends, zero phase: sample 0 maps to sample 0)
 *   src_rate == dst_rate: a plain copy (the filter is not applied).
 * The taps are computed on the host in float64, rounded once to fp32 and cached per (device, up, down); sums are accumulated in
 * fp32, one output per lane in a fixed order: no atomics, two calls are bit-identical and a clip's result does not depend on the
 * batch it is in.  Pass band (44.1 / 48 kHz -> 8 kHz): |gain - 1| < 1e-5 up to 3 kHz; at and above the new Nyquist < -110 dB.
 * Limits: rates >= 1, max(up, down) <= 4096, length >= 1, M < 2^31 (ADN_ERR_INVALID otherwise).
 * audio: device (n_clips, length) fp32; out: device (n_clips, M) fp32, may not alias audio.  adn_resample_prepare builds the tables
 * of a rate pair (adn_resample's and adn_resample_stream's) on `device` ahead of time (synchronous, idempotent, thread-safe); a cold adn_resample on a stream that is being
 * captured enqueues nothing and returns ADN_ERR_INVALID. */
ADN_API int adn_resample_length(long length, int src_rate, int dst_rate, long *out_length);
ADN_API int adn_resample_prepare(int device, int src_rate, int dst_rate);
ADN_API int adn_resample(const float *audio, int n_clips, long length, int src_rate, int dst_rate, float *out, void *stream);
/* add_noise for "white" / "urban" (code/create_train_dataset.py:147-157), clip by clip:
 *   c = sqrt(mean(clean^2) + 1e-12), n = sqrt(mean(noise^2) + 1e-12), s = c / 10^(snr_db / 20) / n,
 *   out = clip(clean + s * noise, -1, 1)
 * (the reference's `noise_rms > 1e-9` branch is always taken because of the 1e-12; silent noise gives s * 0 = 0).
 * clean, noise, out: device (n_clips, length) fp32; out may be `noise` (written in place) but not `clean`.  The two mean
 * squares are blocked fp32 sums in a fixed order (8192-sample blocks spread over the chip, then a tree): no float atomics,
 * two calls are bit-identical.  adn_mix_snr_workspace_bytes of device scratch; snr_db in [-200, 200]. */
ADN_API int adn_mix_snr_workspace_bytes(int n_clips, long length, size_t *bytes);
ADN_API int adn_mix_snr(const float *clean, const float *noise, int n_clips, long length, float snr_db,
                        void *workspace, size_t workspace_bytes, float *out, void *stream);

/* add_noise for "reverb" (code/create_train_dataset.py:87-102,116-121), clip by clip.  The reference renders it with Pedalboard's
 * Reverb, which wraps JUCE's Reverb, which is Freeverb (public domain).  This library DEFINES the effect below; the constants
 * were written down without the JUCE source at hand and have NOT been checked against it: they are this project's effect, and
 * parity with Pedalboard is unpinned (float64 restatement: tests/reverb_ref.py).
 * Mono, every clip on its own, all state zero at the clip's first sample (the reference applies a fresh board to each chunk).
 *   delay lengths D = (sample_rate * tuning) / 44100 in integer arithmetic (rounded down);
 *     comb tunings 1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617; all-pass tunings 556, 441, 341, 225
 *     (8 kHz: combs 202, 215, 231, 245, 257, 270, 282, 293; all-pass 100, 80, 61, 40)
 *   scalars, every operation rounded to fp32, in this order:
 *     feedback = room_size * 0.28 + 0.7;  damp = damping * 0.4;  gain = 0.015;
 *     wet1 = 0.5 * (wet_level * 3) * (1 + width);  dry = dry_level * 2
 *   per sample n, with in = x[n] * gain and acc = 0:
 *     comb j = 0..7 in index order, each with a circular buffer buf_j of D_j zeros and last_j = 0:
 *       o = buf_j[n mod D_j];  last_j = o * (1 - damp) + last_j * damp;  buf_j[n mod D_j] = in + last_j * feedback;  acc += o
 *     all-pass j = 0..3 in series:  b = buf[n mod D];  buf[n mod D] = acc + b * 0.5;  acc = b - acc
 *     y[n] = acc * wet1 + x[n] * dry, then clipped to [-1, 1] when `clip` is nonzero (add_noise clips).
 *   This function has no defaults; the Python mirror's are the reference's call (create_train_dataset.py:94: room_size 0.9,
 *   damping 0.9, wet_level 0.33) plus dry_level 0.4 and width 1.0 for the two it leaves to Pedalboard.
 * Not reproduced: JUCE's parameter smoothing ramps (the parameters are constant over a clip), its denormal nudge, freeze mode
 * and the stereo pair (width only enters wet1).
 * The kernel walks a clip in chunks of min(D) samples: inside a chunk no delay line meets itself, the comb sum and the all-pass
 * chain are element-wise and each comb's low-pass is a wave-level scan v[i] = damp v[i-1] + b[i] with the previous chunk's
 * carry.  That re-associates the low-pass sums only (fp32 throughout; within a few fp32 roundings of the sample-by-sample fp32
 * loop).  No atomics, one fixed order: two calls are bit-identical and a clip's result does not depend on the batch it is in.
 * audio, out: device (n_clips, length) fp32; out may be `audio` (each sample is read before it is written).  No workspace: the
 * twelve delay lines of a clip live in the LDS of its workgroup (9 KB at 8 kHz, 50 KB at 44.1 kHz, 110 KB at 96 kHz).
 * Limits (ADN_ERR_INVALID otherwise, nothing is launched): 2000 <= sample_rate <= 128000 (shortest delay >= 10 samples; state
 * + staging <= 160 KiB); the five parameters in [0, 1] (NaN refused); n_clips >= 1; 1 <= length < 2^30 (sample indices inside a clip are 32-bit; offsets between clips 64-bit). */
ADN_API int adn_reverb(const float *audio, int n_clips, long length, int sample_rate, float room_size, float damping,
                       float wet_level, float dry_level, float width, int clip, float *out, void *stream);

/* ---- inverse STFT and Griffin-Lim ----------------------------------------------------------------------------
 * Replaces griffin_lim_reconstruction (/root/reference/code/test.py:29-48): librosa.istft + librosa.stft iterated
 * from a random-phase start (librosa 0.10 defaults: n_fft = 2*(n_bins-1), periodic Hann, center=True, zero pad,
 * istft length = hop*(n_frames-1), window sum-of-squares normalisation).  As in the reference the target magnitude is
 * NOT re-imposed inside the loop.  `rnd` holds what np.random.rand(F, T) returned (uniform [0,1), as float32).
 * magnitude, rnd: device (n_clips, n_bins, n_frames) fp32 [the reference's (F, T) layout]; audio_out: device
 * (n_clips, hop*(n_frames-1)) fp32.  Complex spectrograms of the building blocks below are FRAME-major:
 * (n_clips, n_frames, n_bins, 2) fp32. */
ADN_API int adn_istft_length(int n_frames, int hop, long *length);
ADN_API int adn_griffin_lim_workspace_bytes(int n_clips, int n_bins, int n_frames, size_t *bytes);
ADN_API int adn_griffin_lim(const float *magnitude, const float *rnd, int n_clips, int n_bins, int n_frames, int n_fft, int hop,
                    int iterations, void *workspace, size_t workspace_bytes, float *audio_out, void *stream);
/* librosa.stft(audio, n_fft, hop) complex result, centred: n_frames = 1 + length/hop (test.py:41-43). */
ADN_API int adn_stft_complex(const float *audio, int n_clips, long length, int n_fft, int hop, float *spec_out, void *stream);
/* librosa.istft(spec, hop_length=hop) (test.py:40,48); workspace = n_clips*n_frames*n_fft floats. */
ADN_API int adn_istft_workspace_bytes(int n_clips, int n_frames, int n_fft, size_t *bytes);
ADN_API int adn_istft(const float *spec, int n_clips, int n_frames, int n_fft, int hop, void *workspace, size_t workspace_bytes,
              float *audio_out, void *stream);

/* ---- denoise: audio of any length through the network and back ---------------------------------------------------------------
 * The reference feeds one fixed 257 x 188 spectrogram per clip to the network (test.py:100-114) and goes back to audio through
 * Griffin-Lim from a random phase (test.py:29-48).  These entry points DEFINE the long form (no reference counterpart; float64
 * restatement in tests/denoise_ref.py): the spectrogram is cut into overlapping windows of the width the network was trained
 * for, the outputs are cross-faded, and the audio comes back with the noisy input's own phase.
 * Not pinned / not validated: parity of the STFT with librosa stays unpinned as for adn_stft_complex; the defaults
 * window = 256, overlap = 32 are design defaults whose audible quality has not been judged (no trained checkpoint exists
 * here); the result of overlapping windows DIFFERS from a forward over the whole spectrogram by design (the network's receptive
 * field is wider than the overlap) -- the single-window case is exact, the multi-window case is what is defined below.
 *
 *   n_fft power of two in [64, 4096], 1 <= hop <= n_fft / 4, F = n_fft / 2 + 1, window W >= 16, overlap 0 <= V <= W / 2, S = W - V.
 *   1. X = adn_stft_complex(x): T = 1 + floor(L / hop) frames, centred, zero padded.
 *   2. Plan (adn_denoise_plan): T <= W: one window of width max(T, 16).  Otherwise K = 1 + ceil((T - W) / S) windows of width W,
 *      window k holds frames [k S, k S + W), frames >= T are zero.  in[k, 0, f, j] = |X[k S + j, f]| with
 *      |X| = sqrtf(fmaf(re, re, im * im))   (one rounded product, one fma, one correctly rounded square root; no fp16 step).
 *   3. y = UNet(in), (K, 1, F, W).
 *   4. Stitch: weight of window k at local frame j: (j + 1) / (V + 1) for j < V and k > 0; (W - j) / (V + 1) for j >= W - V
 *      and k < K - 1; 1 otherwise.  At most two windows cover a frame and their weights sum to 1.
 *      Y[f, t] = sum_k a_k y[k, 0, f, t - k S] in ascending k: fp32 weights (one division), two rounded products, one rounded
 *      sum, never contracted; a frame covered by one window is y itself, bit for bit.  M = max(Y, 0) with clamp (NaN stays NaN,
 *      as in the network's ReLU), Y without.
 *   5. Noisy phase (adn_denoise_resynth, clamp on): S^[t, f] = M[f, t] X[t, f] / |X[t, f]|, S^ = M (real) where the |X| of
 *      rule 2 is 0; x^ = inverse STFT as adn_istft defines it (periodic Hann, overlap-added frames divided by the window
 *      sum-of-squares of the frames that cover a sample, summed in ascending frame order) but of length L like
 *      librosa.istft(..., length=L): the L - hop (T - 1) < hop tail samples are still covered by the last centred frames.
 *      hop <= n_fft / 4 keeps that divisor >= 0.25 over [0, L); at hop = n_fft / 2 it falls to 2e-8 at the last tail sample,
 *      hence the limit.  T = 1 (L < hop) is legal.
 * Layouts: spec is frame-major (n_clips, n_frames, n_bins, 2) fp32 as adn_stft_complex writes it (8-byte aligned); windows /
 * y are (n_clips * K, 1, n_bins, width) fp32, the window's frame index fastest, a clip's K windows consecutive; stitched
 * spectrograms are (n_clips, n_bins, n_frames).  adn_denoise_windows and adn_denoise_stitch take any n_bins >= 1.
 * All three kernels are deterministic (no atomics, fixed summation order): two calls are bit-identical and a clip's result does
 * not depend on the batch it is in.  adn_denoise_resynth needs no workspace: a workgroup owns up to 4096 output samples, recomputes the
 * n_fft / hop - 1 frames it shares with its neighbours, and keeps frames and the stitched magnitudes in LDS; it uses the tables
 * of (device, n_fft) like the STFT family (adn_prepare before a capture).
 * Limits (ADN_ERR_INVALID otherwise): length < 2^30 samples; K * width < 2^31; launch grids < 2^31 workgroups (n_clips x windows
 * x 32x32 tiles; n_clips x n_bins x ceil(n_frames / 1024); n_clips x ceil(length / 2048)).  Element offsets are 64-bit.
 * adn_denoise_plan is host-only (no device needed). */
ADN_API int adn_denoise_plan(int n_frames, int window, int overlap, int *n_windows, int *window_width);
ADN_API int adn_denoise_windows(const float *spec, int n_clips, int n_frames, int n_bins, int window, int overlap, float *out,
                                void *stream);
ADN_API int adn_denoise_stitch(const float *y, int n_clips, int n_frames, int n_bins, int window, int overlap, int clamp,
                               float *out, void *stream);
ADN_API int adn_denoise_resynth(const float *y, const float *spec, int n_clips, long length, int n_fft, int hop, int window,
                                int overlap, float *audio_out, void *stream);

/* ---- stream: audio that is still arriving, in blocks, with the state carried on the device ------------------------------------
 * adn_denoise_* handle a finished recording.  These entry points DEFINE the streaming form (no reference counterpart; float64
 * restatement in tests/stream_ref.py): the "denoise" definition above with rules 2-4 replaced.  Rule 1 (the centred STFT) and
 * rule 5 (clamp, the noisy input's phase, the inverse STFT of the input's full length L) stay as they are.
 * Not pinned / not validated: parity of the STFT with librosa, as everywhere; the quality of the proposed defaults window 192,
 * block 16, look-ahead 0 (design values); equality with the offline form -- the windows differ by design.
 *
 *   n_fft power of two in [64, 4096], 1 <= hop <= n_fft / 4, F = n_fft / 2 + 1, window W >= 16 frames, block B >= 1 frames,
 *   look-ahead A >= 0 frames, B + A <= W.
 *   Frames: frame t is the centred frame of rule 1: samples [t hop - n_fft/2, t hop + n_fft/2), samples before 0 are zero; it is
 *     complete once t hop + n_fft/2 samples have arrived.
 *   Steps: step k = 0, 1, ... feeds the network one window per stream, in[k, 0, f, j] = |X[k B + B + A - W + j, f]| for j < W;
 *     frames < 0 are zero and, after the end, frames >= T are zero; |X| exactly as in rule 2.  Step k can run when frame
 *     k B + B + A - 1 is complete: after m samples steps_done(m) = 0 if r = m - n_fft/2 - (B + A - 1) hop < 0, else r / (B hop) + 1.
 *   Join: Y[f, k B + i] = y[k, 0, f, W - B - A + i] for i < B: every frame comes from exactly one window, bit for bit -- no
 *     cross-fade; the past context provides continuity.  M = max(Y, 0), NaN stays NaN.
 *   Output: after step k the samples n < (k + 1) B hop - n_fft/2 are final: emitted(m) = max(0, steps_done(m) B hop - n_fft/2).
 *   Latency: at worst (B + A - 1) hop + n_fft samples between a sample's arrival and its emission.
 *   End of stream: after L samples in all the remaining steps up to K = ceil(T / B), T = 1 + L / hop, run with the frames that
 *     reach past L zero padded and the frames >= T zero in the windows; the stream has then produced exactly L samples, and they
 *     are rule 5's inverse STFT of M with the phase of X.
 *
 * The library keeps no per-stream host state: the step index is an argument and everything carried between calls lives in a
 * caller-owned device buffer (`state`, adn_stream_state_bytes, 8-byte aligned, opaque; adn_stream_reset before the first step of a
 * stream).  All n_streams streams of a state advance in lockstep.  A call covers the n_steps <= max_steps consecutive steps
 * first_step .. first_step + n_steps - 1; calls go in step order, and the steps a call analyses are emitted before later steps
 * are analysed.  final_length is -1 while the stream runs and L for the steps that run after its end (at most up to step K - 1).
 *   adn_stream_analyze: `audio` holds, per stream (audio_stride floats apart), the samples the steps bring: samples
 *     [e(first_step - 1), e(last_step)) with e(k) = (k B + B + A - 1) hop + n_fft/2 and e(-1) = 0, cut at L when final_length is
 *     given (the pointer must be valid even when that leaves none).  windows_out: (n_streams * n_steps, 1, F, W) fp32, the frame
 *     index fastest, a stream's steps consecutive: the input of adn_unet_forward.
 *   adn_stream_emit: y, the network's output for those windows, same layout.  audio_out, per stream (out_stride floats apart),
 *     receives samples [max(0, first_step B hop - n_fft/2), (last_step + 1) B hop - n_fft/2), or up to L when last_step = K - 1
 *     with final_length given; it may be NULL when that range is empty (B hop < n_fft/2 in the first steps).
 * Two launches analyse (new frames into the state, then the windows out of it), one emits.  No atomics, no workspace; a sample
 * is the carried partial sum plus its frames in ascending frame order, so the same audio gives the same bits however it was
 * split into calls and a stream's result does not depend on its neighbours in the batch.  At the start of a stream and after its
 * end the divisor is adn_denoise_resynth's.  The kernels use the tables of (device, n_fft) like the STFT family: adn_prepare
 * before a capture (a cold call on a capturing stream enqueues nothing and returns ADN_ERR_INVALID).
 * Limits (ADN_ERR_INVALID otherwise, nothing is launched): the parameter ranges above; n_streams >= 1; 1 <= max_steps <= 65536;
 * n_steps <= max_steps; the steps of a call end before sample 2^30 of the stream (positions are 32-bit inside the kernels: flush
 * before that, 37 hours at 8 kHz).  ADN_ERR_WORKSPACE: state_bytes below adn_stream_state_bytes.
 * adn_stream_plan (steps_done, emitted and latency for `received` samples; any output pointer may be NULL) and
 * adn_stream_state_bytes are host-only (no device needed). */
ADN_API int adn_stream_plan(int n_fft, int hop, int window, int block, int lookahead, long received, long *steps_done,
                            long *emitted, long *latency);
ADN_API int adn_stream_state_bytes(int n_streams, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                                   size_t *bytes);
ADN_API int adn_stream_reset(void *state, size_t state_bytes, int n_streams, int n_fft, int hop, int window, int block,
                             int lookahead, int max_steps, void *stream);
ADN_API int adn_stream_analyze(void *state, size_t state_bytes, const float *audio, long audio_stride, int n_streams,
                               long first_step, int n_steps, long final_length, int n_fft, int hop, int window, int block,
                               int lookahead, int max_steps, float *windows_out, void *stream);
ADN_API int adn_stream_emit(void *state, size_t state_bytes, const float *y, int n_streams, long first_step, int n_steps,
                            long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                            float *audio_out, long out_stride, void *stream);

/* ---- stream pool: streams that start, stop and advance independently, their ready steps batched ---------------------------------
 * These entry points DEFINE the pool as n_slots independent instances of the stream definition above: there is no new arithmetic.
 * The stream in a slot has its own step index and its own end; what it returns is a function of its own samples and its own step
 * index only, bit for bit what adn_stream_analyze / adn_stream_emit return for a state of one stream (n_streams = 1) that runs
 * the same steps one per call.  Not claimed: anything about the order or the timing in which a caller serves its streams.
 *
 * State (adn_stream_pool_state_bytes, caller-owned, opaque, 8-byte aligned): per slot the sections of a stream state with
 * max_steps = 1 -- X, (B + A) F complex frames; mag, W F magnitudes; tail, 2 (n_fft - hop) partial sums -- and, in place of the
 * history section, a RING of ring_samples pending samples, sample s of the slot's stream at s mod ring_samples:
 *   floats = n_slots (2 (B + A) F + W F + 2 (n_fft - hop) + ring_samples), F = n_fft / 2 + 1.
 * adn_stream_pool_reset clears one slot, or all for slot = -1.  A stream that starts at step 0 reads nothing an earlier stream
 * of its slot has left, so a slot may be reused without a reset.
 *   adn_stream_pool_write: the n samples of the stream in `slot` from absolute position `position` on (audio, device memory) go
 *     into its ring, the wrap handled inside: at most two device copies.  0 <= n <= ring_samples, position >= 0.
 *   adn_stream_pool_analyze: `rows`, a HOST array read during the call, names n_rows (slot, step, final_length): row i runs step
 *     `step` of the stream in `slot`, final_length as in adn_stream_analyze (-1 while that stream runs).  windows_out:
 *     (n_rows, 1, F, W) fp32, window i from row i: the input of adn_unet_forward.  CONTRACT of the caller: the ring of the slot
 *     holds the samples [e(step - 1) - (n_fft - hop), e(step)) of its stream (cut at 0 and at final_length) when the call runs.
 *   adn_stream_pool_emit: the same rows; y, the network's output for those windows.  Row i's samples go to
 *     audio_out + i out_stride: as many as adn_stream_emit returns for (step, 1, final_length).  out_stride >= B hop + n_fft/2,
 *     the most a step emits (the last one of a stream).
 * A slot's steps go in step order, and a step is emitted before the slot's next one is analysed, as in the stream section.
 * The kernels are the stream section's, the rows handed to them by value in the kernel arguments (no host -> device copy, no
 * workspace, no atomics); no state word is written by one workgroup and read by another in the same launch, for which a call
 * must not name a slot twice.  Cold-call and capture behaviour as for adn_stream_analyze / adn_stream_emit.
 * Limits (ADN_ERR_INVALID otherwise, nothing is launched): the stream section's, applied to every row with n_steps = 1;
 * 1 <= n_rows <= ADN_STREAM_POOL_MAX_ROWS (a caller with more ready streams calls again); 0 <= slot < n_slots; no slot twice in
 * a call; ring_samples >= (n_fft - hop) + (B + A - 1) hop + n_fft/2 + B hop (what the first step reads and one block more) and
 * <= 2^28; 1 <= n_slots <= 2^20.  ADN_ERR_WORKSPACE: state_bytes below adn_stream_pool_state_bytes.
 * adn_stream_pool_state_bytes is host-only (no device needed). */
#define ADN_STREAM_POOL_MAX_ROWS 256
typedef struct adn_stream_pool_row {
    int slot;
    int step;
    int final_length;
} adn_stream_pool_row;
ADN_API int adn_stream_pool_state_bytes(int n_slots, int n_fft, int hop, int window, int block, int lookahead, long ring_samples,
                                        size_t *bytes);
ADN_API int adn_stream_pool_reset(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                  int lookahead, long ring_samples, int slot, void *stream);
ADN_API int adn_stream_pool_write(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                  int lookahead, long ring_samples, int slot, const float *audio, long n, long position,
                                  void *stream);
ADN_API int adn_stream_pool_analyze(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                    int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows,
                                    float *windows_out, void *stream);
ADN_API int adn_stream_pool_emit(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                 int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, const float *y,
                                 float *audio_out, long out_stride, void *stream);

/* ---- resample stream: adn_resample for audio that is still arriving ----------------------------------------------------------------
 * The resampler definition above (up, down, q, half = 32 q, the taps h, y[m] = sum_i x[i] h[m down - i up] with zero extension)
 * with a finality rule added (float64 restatement: tests/stream_resample_ref.py).  For a stream that has received n input samples:
 *   Running: output m is final once every input it reads has arrived, m down + half < n up:
 *     emitted(n) = 0 if n up <= half, else floor((n up - half - 1) / down) + 1.
 *   Ended at length L: emitted = ceil(L up / down); inputs from L on are zero, exactly as in adn_resample.
 *   Carried samples: at most H = 2 floor(half / up) + ceil(down / up) + 1 input samples have to survive a call.
 *   Latency: n - emitted(n) down / up <= half / up for every n: latency = ceil(half / up) input samples, 4 ms at every audio rate pair.
 *   Equal rates: a copy, no state read or written (its size is 0, the pointer may be NULL), emitted(n) = n, H = latency = 0.
 * Arithmetic: one output per lane, acc = 0, then acc = fmaf(x[i], h32, acc) over the output's own window in ascending i, with the
 * fp32 taps adn_resample uses.  That is the chain adn_resample runs (its further steps carry zero coefficients or zero samples
 * and leave a finite accumulator unchanged): the outputs of a stream are, bit for bit, adn_resample's of the finished signal,
 * however it was cut into calls; a stream's result does not depend on its neighbours in the batch.  No atomics, no workspace.
 *
 * The library keeps no per-stream host state: everything a call needs follows from its arguments and the caller-owned, opaque,
 * 8-byte-aligned `state` (adn_resample_stream_state_bytes: two slots of H samples per stream).  One call = the next n_new samples of
 * every one of the n_streams streams (`audio`, audio_stride floats apart), one kernel launch.  call_index is the number of earlier
 * calls of this stream and received_before the samples they brought; call 0 reads no state, so a new stream needs no reset.
 * final = 1 marks the last call (n_new may then be 0, and audio NULL).  The call writes, per stream (out_stride floats apart), the
 * outputs [emitted(received_before), emitted(received_before + n_new, final)); `out` may be NULL when that range is empty.
 * Limits (ADN_ERR_INVALID before any HIP call): the rate limits of adn_resample; H <= 16384 (192 kHz -> 8 kHz: 1561; excluded are
 * ratios such as 4096:1, whose single output reads 262 145 inputs); n_streams >= 1; n_new >= 1 unless final; call_index >= 0 and
 * call_index == 0 exactly when received_before == 0; input and output positions < 2^31; null pointers; strides below the samples
 * of a call when n_streams > 1.  ADN_ERR_WORKSPACE: state_bytes below adn_resample_stream_state_bytes.
 * adn_resample_prepare builds this entry point's coefficient table too; a cold call on a capturing stream enqueues nothing and
 * returns ADN_ERR_INVALID, a warm call only enqueues.  adn_resample_stream_plan (emitted for `received` samples, H and the latency;
 * any output pointer may be NULL) and adn_resample_stream_state_bytes are host-only (no device needed). */
ADN_API int adn_resample_stream_plan(int src_rate, int dst_rate, long received, int final, long *emitted, long *history,
                                     long *latency);
ADN_API int adn_resample_stream_state_bytes(int n_streams, int src_rate, int dst_rate, size_t *bytes);
ADN_API int adn_resample_stream(void *state, size_t state_bytes, const float *audio, long audio_stride, int n_streams,
                                long call_index, long received_before, long n_new, int final, int src_rate, int dst_rate,
                                float *out, long out_stride, void *stream);

/* ---- stream pool at a rate: the pool's streams resampled into their rings and back, all rows of a call in one launch ------------
 * These entry points define no new arithmetic: a ROW is one adn_resample_stream call of one stream, and a row's outputs are, bit
 * for bit, adn_resample_stream's for a state of one stream (n_streams = 1) given the same calls -- hence adn_resample's of the
 * finished signal, however it was cut.  What is new is where the rows come from and go to: every row names its own slot, rate,
 * call_index, received_before, n_new and final (their meaning and the finality rule: "resample stream" above), the table is
 * handed to one kernel launch by value (no host -> device copy, no workspace, no atomics), and a row's outputs go either into the
 * slot's ring inside a pool state or to a row of a plain buffer.  work_rate is the rate of the pool's rings.
 *
 * Rate state (adn_stream_pool_rate_state_bytes, caller-owned, opaque, 8-byte aligned, separate from the pool state, whose layout
 * and size do not change): per slot and DIRECTION (0: into the pool, 1: out of it) two slots of max_history floats,
 *   floats = n_slots * 2 * 2 * max_history,
 * used as adn_resample_stream uses its state: call 0 of a stream reads none of it, so a slot is reused without a reset, at
 * another rate too.  max_history >= the H of every rate pair the state is used with (adn_resample_stream_plan).
 *   adn_stream_pool_push_rate: row i brings the next n_new samples of the stream in `slot`, at src_rate, found at
 *     audio + audio_offset (ONE device buffer holds the blocks of all rows); direction 0.  Its outputs at work_rate, the samples
 *     [emitted(received_before), emitted(received_before + n_new, final)) of the stream, go to the words m mod ring_samples of the
 *     slot's ring; a range that straddles the wrap is handled in the kernel.  The first arguments are the pool state and its
 *     geometry, as in the "stream pool" section.  CONTRACT of the caller: the ring has room for them (no step still reads the
 *     words they replace).
 *   adn_stream_pool_emit_rate: row i takes the stream in `slot` from work_rate to dst_rate (`rate`); direction 1.  It reads n_new
 *     samples at audio_in + i in_stride + audio_offset -- with audio_offset = 0 the layout adn_stream_pool_emit writes; a caller
 *     that leaves rows of that buffer out (streams at work_rate, steps that returned nothing) names the rows it skipped there, so
 *     that any subset of a tick's rows is one call -- and writes its outputs from out + i out_stride on.
 * Equal rates are a copy that reads and writes no history.  No state word is written by one workgroup and read by another in
 * the same launch, for which a call must not name a (slot, direction) twice.
 * Limits (ADN_ERR_INVALID before any launch): for every row everything adn_resample_stream refuses -- the rate limits,
 * n_new >= 1 unless final, final 0 or 1, call_index >= 0 and call_index == 0 exactly when received_before == 0, positions < 2^31;
 * H of the row's rate pair <= max_history <= 16384; 0 <= slot < n_slots, 1 <= n_slots <= 2^20; the same slot twice in a call;
 * 1 <= n_rows <= ADN_STREAM_POOL_RATE_MAX_ROWS (a caller with more rows calls again); audio_offset >= 0; null pointers;
 * push: more outputs than ring_samples in one row, outputs at or beyond sample 2^30 of the stream (the pool's limit), the pool
 * section's limits on the state and its geometry; emit: in_stride below a row's n_new or out_stride below its outputs when
 * n_rows > 1.  ADN_ERR_WORKSPACE: rate_state_bytes below adn_stream_pool_rate_state_bytes (or the pool state below its size).
 * Cold coefficient tables behave as in adn_resample_stream: adn_resample_prepare(device, src, dst) warms them; a cold call on a
 * capturing stream enqueues nothing and returns ADN_ERR_INVALID.  adn_stream_pool_rate_state_bytes is host-only. */
#define ADN_STREAM_POOL_RATE_MAX_ROWS 64
typedef struct adn_stream_pool_rate_row {
    int slot;
    int rate;              /* push: src_rate; emit: dst_rate */
    long call_index;
    long received_before;
    long n_new;
    int final;
    long audio_offset;     /* floats from `audio` (push) or from audio_in + i in_stride (emit) to the row's samples */
} adn_stream_pool_rate_row;
ADN_API int adn_stream_pool_rate_state_bytes(int n_slots, int max_history, size_t *bytes);
ADN_API int adn_stream_pool_push_rate(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                      int lookahead, long ring_samples, void *rate_state, size_t rate_state_bytes, int max_history,
                                      int work_rate, const adn_stream_pool_rate_row *rows, int n_rows, const float *audio,
                                      void *stream);
ADN_API int adn_stream_pool_emit_rate(void *rate_state, size_t rate_state_bytes, int n_slots, int max_history, int work_rate,
                                      const adn_stream_pool_rate_row *rows, int n_rows, const float *audio_in, long in_stride,
                                      float *out, long out_stride, void *stream);

/* ---- quality: objective metrics of an estimate against a clean reference, clip by clip ------------------------------------------
 * No reference counterpart (the reference judges by ear and by its training loss).  The library DEFINES the operators below; the
 * float64 restatement is tests/quality_ref.py.  est, ref: device (n_clips, length) fp32, `length` the row pitch in samples.
 * lengths: device array of n_clips `long`, or NULL = every clip is `length` long; it is read ON THE DEVICE (no host
 * synchronisation), each value is taken as min(max(value, 0), length), and no sample at or beyond a clip's own length is read.
 * Results are fp32, one row per clip.  Nothing is allocated and nothing blocks; no constant table is needed (a capture may hold a
 * first call).  No atomics, one fixed order of summation laid out by sample position inside the clip: two calls are bit-identical,
 * a clip's result is bit-identical whatever batch it sits in, and a row cut by `lengths` equals the same clip passed unpadded.
 * Workspaces: 16-byte aligned (ADN_ERR_INVALID otherwise), ADN_ERR_WORKSPACE below the size function's bytes.
 * Limits (ADN_ERR_INVALID before any launch): n_clips >= 1, 1 <= length < 2^30, launch grids < 2^31 workgroups, null est / ref / out.
 *
 * adn_quality: out (n_clips, 3) = {SNR, SI-SDR, segmental SNR} in dB.  With e = est, r = ref over the clip's own samples:
 *   SNR     = 10 log10(Srr / Sdd),  Srr = sum r^2,  Sdd = sum (e - r)^2
 *   SI-SDR  = 10 log10( sum (alpha r)^2 / sum (e - alpha r)^2 ),  alpha = Ser / Srr,  Ser = sum e r.  The residual sum is
 *             accumulated from the per-sample differences in a second pass over the audio once alpha is known -- never as
 *             sum e^2 - Ser^2 / Srr, which loses everything above about 60 dB in fp32.
 *   segSNR  = mean over the floor(len / seg_frame) whole, non-overlapping frames of seg_frame samples of
 *             clamp(10 log10((Srr_f + 1e-10) / (Sdd_f + 1e-10)), -10, 35);  16 <= seg_frame <= 8192 (the Python mirror's default is
 *             int(0.03 * sample_rate)); a trailing partial frame is not counted; with no whole frame the result is NaN.
 *   Accumulation: fp64 everywhere.  A sample is widened to fp64 first (products and differences of fp32 values are then exact),
 *   a block of 8192 samples is summed by 256 lanes of 32 strided fma terms each and a fixed tree, a frame likewise by 64 lanes (16
 *   below 64 samples); the block sums of a clip, alpha, the ratios and the logarithms are fp64, and each result is rounded to fp32
 *   once.  The audio is read twice (four array reads); the segmental frames are summed in the first pass.
 *   Degenerate inputs follow IEEE arithmetic: est == ref gives +inf for SNR and SI-SDR (any ratio x / 0, x > 0); a silent ref with
 *   a non-zero error gives -inf for SNR and NaN for SI-SDR (alpha = 0 / 0); a clip of length 0 gives NaN three times.
 *
 * adn_stoi: out (n_clips,) = the short-time objective intelligibility measure of Taal, Hendriks, Heusdens and Jensen (2011), for
 * audio ALREADY AT 10 kHz (the rate conversion is the caller's; the Python mirror uses adn_resample).  The definition below is
 * this project's own statement of it and is UNPINNED against pystoi, which no machine of this project has.
 *   Constants: frame 256, hop 128, FFT 512, 15 bands, segment N = 30, beta = -15 dB, dynamic range 40 dB;
 *   window w = numpy.hanning(258)[1:-1] (256 values);  EPS = 2^-52.
 *   1. Frames.  Start positions range(0, L - 256, 128) -- the bound is exclusive, so L = 256 + 128 k yields k frames, not k + 1.
 *      x_i = w . ref[s_i : s_i + 256], and the same for est.
 *   2. Silent-frame removal, decided on ref alone.  E_i = 20 log10(||x_i||_2 + EPS); frame i is kept when E_i > max_i E_i - 40.
 *      idx[0..K) are the kept frames in order.
 *   3. Compacted signals: the overlap-add of the kept windowed frames at hop 128, for ref and est:
 *        c[n] = sum over j in {floor(n / 128) - 1, floor(n / 128)}, 0 <= j < K, of w[n - 128 j] . sig[128 idx[j] + n - 128 j],
 *      of length 128 (K + 1).
 *   4. Spectra of the compacted signals.  The same framing rule applied to c gives exactly J = K - 1 frames; each is windowed by w
 *      again, zero padded to 512 and takes a real FFT to 257 bins; |X|^2 is kept.
 *   5. One-third-octave envelopes.  X_tob[b, j] = sqrt(sum over k in [lo_b, hi_b) of |X[k, j]|^2), and the same for est.  The bin
 *      ranges follow from f = linspace(0, 10000, 513)[:257], centres 150 . 2^(b/3), edges 150 . 2^((2b -+ 1)/6), nearest bin by
 *      squared distance:  (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138)
 *      (138,174) (174,219).
 *   6. Per segment and band.  For every m = 30 ... J inclusive and every band, over the 30 frames [m - 30, m), x of ref, y of est:
 *      a = ||x|| / (||y|| + EPS);  y' = min(a . y, x . (1 + 10^(15/20)));  the mean of x and of y' over the 30 frames is removed;
 *      each is divided by its norm plus EPS;  rho = sum x^ y^'.
 *   7. Result.  d = sum rho / (15 . (J - 29)).  If J < 30, that is K < 31, d = NaN -- pystoi returns 1e-5 with a warning there.
 *   Arithmetic: the window is computed in fp64 and rounded once to fp32; steps 1-5 are fp32 (frame norms: four fma terms per lane
 *   and a wave tree; the 512-point transform as 256 packed complex points on the library's Stockham passes; band sums in ascending
 *   bin order); the comparison of step 2 is made on the norms, n_i + EPS > (n_max + EPS) / 100, in fp64; steps 6 and 7 are fp64,
 *   the correlations of a clip added in a fixed order.  A frame whose E_i lies within rounding of the threshold may fall on either
 *   side of it; everything else is continuous in the input.  The compacted signals are never stored: each of their frames is
 *   built from the source frames idx[j - 1], idx[j], idx[j + 1], and only the 2 x 15 envelopes per frame reach the workspace. */
ADN_API int adn_quality_workspace_bytes(int n_clips, long length, size_t *bytes);
ADN_API int adn_quality(const float *est, const float *ref, const long *lengths, int n_clips, long length, int seg_frame,
                        void *workspace, size_t workspace_bytes, float *out, void *stream);
ADN_API int adn_stoi_workspace_bytes(int n_clips, long length, size_t *bytes);
ADN_API int adn_stoi(const float *est, const float *ref, const long *lengths, int n_clips, long length, void *workspace,
                     size_t workspace_bytes, float *out, void *stream);

/* ---- baseline: a classical spectral denoiser that needs no weights ---------------------------------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement: tests/baseline_ref.py);
 * it is UNPINNED against any package.  The recursions are Doblinger's continuous minimum tracking (1995) for the noise power,
 * Ephraim and Malah's decision-directed a-priori SNR (1984) and a Wiener gain with a floor.  It is causal and carries three floats
 * per bin.  Its place: real denoised audio without a trained network, and the figure a trained network has to beat.
 * Not validated: the defaults are the values of the host prototype; they were not tuned by ear.
 *
 * Every (clip, bin) row is independent.  Over its frames t = 0 ... T-1, in fp32, with X the row's complex values:
 *   p_t  = fmaf(re, re, im * im)                      (the |X|^2 of rule 2 of "denoise", before the square root)
 *   first frame of a row:   P_t = p_t,  Pmin_t = p_t,  S_{t-1} = 0
 *   otherwise:              P_t    = a_s P_{t-1} + (1 - a_s) p_t
 *                           Pmin_t = Pmin_{t-1} < P_t ?  g Pmin_{t-1} + ((1 - g) / (1 - b)) (P_t - b P_{t-1})  :  P_t
 *   N_t  = max(bias Pmin_t, 1e-30)
 *   xi_t = (alpha S_{t-1}) / N_t + (1 - alpha) max(p_t / N_t - 1, 0)
 *   G_t  = max(xi_t / (1 + xi_t), g_min)
 *   M_t  = G_t sqrtf(p_t)                             (the output magnitude)
 *   S_t  = (G_t G_t) p_t
 * max(x, c) is `x < c ? c : x`: a NaN x stays NaN.  The parameters are the fp32 values of the struct; 1 - a_s, (1 - g) / (1 - b)
 * and 1 - alpha are computed from them once, in fp32.  Divisions and the square root are correctly rounded.
 * Parameters (adn_spectral_params; NULL = the defaults): smooth a_s 0.7, beta b 0.96, gamma g 0.998, alpha 0.98, gain_floor g_min
 * 0.1, bias 1.0.  Legal (ADN_ERR_INVALID otherwise, nothing is launched; a NaN is illegal): 0 <= smooth, beta, alpha < 1;
 * 0 < gamma < 1; 0 < gain_floor <= 1; 0 < bias <= 100.
 * Non-finite input: a non-finite p_t poisons its own (clip, bin) row from that frame on (NaN magnitudes, NaN state), and nothing
 * else.  An all-zero row gives zeros.
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_baseline.py: per clip
 * max |M - M64| <= 4 FLOOR max M64, FLOOR the error of the same statements run in fp32 on the host); it is NOT pinned bit for bit to
 * numpy.  Beside that, every (clip, bin) is bounded against its own level (tests/recursive_bounds.py):
 * E = max_t |M - M64| / max_t M64 <= 4 floor, and every entry of the state likewise against its own float64 value (a reference
 * entry of 0 has to be exactly 0).  The floor is the case's own: the largest E of the fp32 restatement on the very spectrogram the
 * device ran on, over every bin of the case's three clips, measured when the test runs, never below 2^-23, never a device figure
 * and never above 1e-4 (a case whose floor is, bounds nothing and is not in the grid).  The same bound holds a spectrogram tilted
 * by 80 dB over the bins.  Pinned bit for bit: the result does not depend on how a row's frames were cut into calls (the state
 * carried from call to call), and it does not depend on which batch the clip is in; and, every rule being a ratio or homogeneous
 * in p_t, a power of two per bin on the input comes back as that factor on M and its square on the state, while no square leaves
 * fp32's normal range and N_t stays above its 1e-30.  Every frame goes through one step, compiled with fp contraction off.
 * Deterministic: no atomics, two calls are bit-identical.
 *
 * Layouts: spec is frame-major (n_clips, n_frames, n_bins, 2) fp32 as adn_stft_complex writes it (8-byte aligned).  out is
 * (n_clips, 1, n_bins, width) fp32, the network-output layout adn_denoise_resynth reads: the call writes columns
 * [col0, col0 + n_frames) of every row and not one byte else -- zeroing padding columns is the caller's job.  State:
 * (n_clips, 3, n_bins) fp32, the rows P, Pmin, S of the last frame.  state_in NULL: every row starts fresh; a row whose P is
 * negative starts fresh as well, so one batch can hold clips that start and clips that continue.  state_out may be NULL (the
 * state is dropped) and may equal state_in (each row is read before it is written, by the lane that writes it); otherwise spec,
 * out and the states may not overlap.
 * Cost: one launch, n_clips x ceil(n_bins / 64) waves that each walk their frames in order; 12 n_clips n_frames n_bins bytes.  No
 * workspace, no atomics, no constant table (a capture may hold a first call); nothing blocks or allocates.
 * Limits (ADN_ERR_INVALID before any launch): n_clips, n_frames, n_bins >= 1; col0 >= 0, col0 + n_frames <= width; launch grid
 * n_clips x ceil(n_bins / 64) < 2^31 workgroups.  Element offsets are 64-bit.
 *
 * The magnitude form (adn_spectral_gain_windows: what the stream classes feed).  The input is a magnitude m_t >= 0 instead of a
 * complex value, and the operator is the definition above applied to X_t = m_t + 0i, with no new arithmetic:
 *   p_t = fmaf(m, m, 0 * 0) = round(m * m),   M_t = G_t sqrtf(p_t),   every other rule unchanged.
 * The device runs it through the same one step as adn_spectral_gain, so the result equals, bit for bit, adn_spectral_gain on the
 * same magnitudes rearranged to frame-major (m, 0); tests/baseline_ref.py stays its float64 restatement, called with
 * m.astype(complex).  Streaming gains are therefore NOT bit-equal to the offline gains of the same audio: the stream hands over
 * |X| = sqrtf(p), and sqrtf(p)^2 != p in the last bits.
 * Layouts: windows and y are (n_rows * n_steps, 1, n_bins, window) fp32 with the frame fastest and a row's steps consecutive --
 * what adn_stream_analyze / adn_stream_pool_analyze write and adn_stream_emit / adn_stream_pool_emit read.  Row i, bin f is one
 * recurrence over the frames t = s n_cols + j, s < n_steps, j < n_cols: m_t = windows[i n_steps + s, 0, f, col0 + j], and M_t
 * goes to the same index of y.  The call writes those columns of y and not one byte else; y may equal windows (every element is
 * read before it is written), no other overlap is allowed.  The stream classes call it with col0 = W - B - A and n_cols = B,
 * the only columns adn_stream_emit reads.
 * State: (n_slots, 3, n_bins) fp32, read and written in place by the lane that owns the row.  rows NULL: row i uses slot i and
 * continues; a row whose P is negative starts fresh, as above.  Otherwise rows is a HOST array read during the call and handed to
 * the kernel by value, as the pool's tables are: row i uses rows[i].slot, and with rows[i].fresh != 0 it starts fresh whatever
 * the slot holds -- which lets a pool slot be reused without a reset (fresh = (step == 0)).  Slots no row names are not touched.
 * Pinned bit for bit, besides the equality above: the result does not depend on how a row's frames are cut into calls or steps,
 * on which rows share the call, or on which slot the state sits in.
 * Cost: one launch, n_rows x ceil(n_bins / 64) waves; no workspace, no atomics, no table (a capture may hold a first call).
 * Limits (ADN_ERR_INVALID before any launch): no NULL or misaligned (4-byte) windows, y, state; every count >= 1; col0 >= 0,
 * col0 + n_cols <= window; n_rows <= n_slots without rows; n_rows <= ADN_SPECTRAL_MAX_ROWS with rows, every slot in [0, n_slots)
 * and named once; n_steps x n_cols < 2^31; n_rows x ceil(n_bins / 64) < 2^31; the parameters as above.
 * Not here: log-MMSE gains, any phase but the noisy one. */
typedef struct { float smooth, beta, gamma, alpha, gain_floor, bias; } adn_spectral_params;
ADN_API int adn_spectral_gain(const float *spec, int n_clips, int n_frames, int n_bins, const adn_spectral_params *params,
                              const float *state_in, float *state_out, float *out, int width, int col0, void *stream);
#define ADN_SPECTRAL_MAX_ROWS 256
typedef struct adn_spectral_row { int slot; int fresh; } adn_spectral_row;
ADN_API int adn_spectral_gain_windows(const float *windows, float *y, int n_rows, int n_steps, int n_bins, int window,
                                      int col0, int n_cols, const adn_spectral_params *params,
                                      float *state, int n_slots, const adn_spectral_row *rows, void *stream);

/* ---- dereverb: weighted prediction error per frequency bin, no weights ----------------------------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement: tests/dereverb_ref.py);
 * it is UNPINNED against any package.  It is single-channel WPE, delayed linear prediction per frequency bin with the variance
 * re-estimated from the last result (Nakatani et al. 2010).  Reverberation is a filter, and no gain per bin ("baseline") undoes a
 * filter: this is the classical operator for the "reverb" noise type, and a front end to the gain of "baseline".
 * Not validated: the defaults are the values of the host prototype; they were not tuned by ear.
 *
 * Every (clip, bin) row is independent.  X_t are the row's complex values, t = 0 ... T-1, and X_t = 0 for t < 0.  In fp32:
 *   p_t   = fmaf(re, re, im * im)
 *   phi   = max(rho (sum_t p_t) / T, 1e-30)
 *   d^(0) = X
 *   for i = 1 ... I:
 *       lam_t = max(|d^(i-1)_t|^2, phi),  w_t = 1 / lam_t                       (|.|^2 as p_t above)
 *       R_jk  = sum_t (w_t X_{t-D-j}) conj(X_{t-D-k})                           j, k = 0 ... K-1
 *       P_j   = sum_t (w_t X_{t-D-j}) conj(X_t)
 *       A     = R + ((delta tr(R)) / K + 1e-30) I                               (tr(R) = sum_j Re R_jj, j ascending; A_jj is real)
 *       solve A g = P by Cholesky: A = L L^H column by column, L y = P, L^H g = y
 *       d^(i)_t = X_t - sum_j conj(g_j) X_{t-D-j}                               (j ascending over the taps with t - D - j >= 0)
 *   output d^(I); optional magnitude M_t = sqrtf(fmaf(dre, dre, dim * dim))
 * The weight is applied once, as the product w_t X_{t-D-j} (each component rounded), before the multiply-add with the conjugate;
 * complex multiply-adds are two fmaf per component.  max(x, c) is `x < c ? c : x`: a NaN x stays NaN.  Divisions and square roots
 * are correctly rounded.  The sums over t run in a fixed order that is the implementation's own (the device: frame after frame from
 * t = 0; phi: the partial sums of the frames t = q mod LPB chunk by chunk, added for q ascending, LPB = 16, 32 or 64 from K alone);
 * the order does not depend on the batch or on which bins share the call.  Inner sums of the factorisation and the substitutions
 * run over k ascending (k descending in L^H g = y).
 * Parameters (adn_wpe_params; NULL = the defaults): taps K 20, delay D 3, iterations I 3, loading delta 1e-3, power_floor rho 1e-3.
 * Legal (ADN_ERR_INVALID otherwise, before any launch, the message names the field; a NaN is illegal): 1 <= taps <= 32;
 * 1 <= delay <= 8; 1 <= iterations <= 8; 1e-6 <= loading <= 1; 0 < power_floor <= 1.
 * Consequences: a row with T <= D comes back bit for bit (no tap has a frame); the first D frames of any row come back bit for
 * bit; an all-zero row gives zeros (A = 1e-30 I, P = 0).  A non-finite value is confined to its own (clip, bin) row, whose content
 * is then unspecified.
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_dereverb.py: per clip
 * max |d - d64| <= 4 FLOOR max |d64|, FLOOR the error of the same statements run in fp32 on the host); it is NOT pinned bit for bit
 * to numpy.  Pinned bit for bit: two calls give the same result; a clip gives the same bits alone or in any batch; a bin gives the
 * same bits whichever other bins are in the call.  Deterministic: no atomics.
 *
 * Layouts: spec and spec_out are frame-major (n_clips, n_frames, n_bins, 2) fp32 as adn_stft_complex writes it, 8-byte aligned;
 * they may not overlap.  mag_out may be NULL; otherwise it is (n_clips, 1, n_bins, width) fp32 with width >= n_frames, the
 * network-output layout adn_denoise_resynth reads.  The call writes columns [0, n_frames) of mag_out, all of spec_out and not one
 * byte else -- zeroing padding columns is the caller's job.  It may use the workspace and only the workspace;
 * adn_wpe_workspace_bytes reports 0 today (R, P, the factor and the taps of a row stay on chip), and workspace may then be NULL.
 * Cost: one launch for all iterations, n_clips x ceil(n_bins / B) workgroups, B = 16 bins up to K = 20, 8 up to K = 28, 4 beyond;
 * a clip's frames pass through LDS in chunks, so no limit on n_frames comes from LDS.  No atomics, no constant table (a capture
 * may hold a first call); nothing blocks or allocates.
 * Limits (ADN_ERR_INVALID before any launch): NULL or misaligned spec / spec_out / mag_out; n_clips, n_frames, n_bins >= 1;
 * width >= n_frames with a mag_out; overlapping spec and spec_out; launch grid < 2^31 workgroups; the parameters as above.
 * ADN_ERR_WORKSPACE: workspace_bytes below adn_wpe_workspace_bytes.  Element offsets are 64-bit.
 * For audio that is still arriving, online / recursive WPE: the section after next, "dereverb stream".
 * Not here: more than one channel treated jointly (the next section, "dereverb multichannel"); any tuning by ear. */
typedef struct adn_wpe_params { int taps, delay, iterations; float loading, power_floor; } adn_wpe_params;
ADN_API int adn_wpe_workspace_bytes(int n_clips, int n_frames, int n_bins, const adn_wpe_params *params, size_t *bytes);
ADN_API int adn_wpe(const float *spec, int n_clips, int n_frames, int n_bins, const adn_wpe_params *params, void *workspace,
                    size_t workspace_bytes, float *spec_out, float *mag_out, int width, void *stream);

/* ---- dereverb multichannel: joint WPE of the channels of a recording ---------------------------------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement:
 * tests/dereverb_mc_ref.py); it is UNPINNED against any package.  It is multichannel WPE (Nakatani et al. 2010; Yoshioka and
 * Nakatani 2012): the late reverberation of every channel is predicted from the past frames of ALL channels of the recording, with
 * one variance per frame shared by the channels.  A second microphone sees the same source through another filter, which is what
 * makes the joint prediction remove more than C separate ones (host figures: profiles/bench_dereverb_mc.md).
 * Not validated: the defaults are design values taken from those host figures; they were not tuned by ear.
 *
 * A group is the C channels of one recording, 1 <= C <= 8; every (group, bin) is independent.  X_{t,c} is channel c at frame t,
 * zero for t < 0.  The stacked vector has N = C K entries, x~_t[r] = X_{t-D-j, c} at r = c K + j: channel-major, the lag ascending
 * inside a channel.  In fp32, with the rounding rules of "dereverb" (the weight applied once as w_t x~_t[r], each component
 * rounded; complex multiply-adds as two fmaf per component; max(x, c) as `x < c ? c : x`; correctly rounded division and square
 * root):
 *   p_{t,c} = fmaf(re, re, im * im)
 *   phi     = max(rho (sum_c sum_t p_{t,c}) / (T C), 1e-30)                     (c ascending; a channel's sum as "dereverb" forms it)
 *   d^(0)   = X
 *   for i = 1 ... I:
 *       lam_t = max((sum_c |d^(i-1)_{t,c}|^2) / C, phi),  w_t = 1 / lam_t       (c ascending)
 *       R_rs  = sum_t (w_t x~_t[r]) conj(x~_t[s])                               N x N Hermitian
 *       P_rc  = sum_t (w_t x~_t[r]) conj(X_{t,c})                               N x C
 *       A     = R + ((delta tr(R)) / N + 1e-30) I                               (tr(R) = sum_r Re R_rr, r ascending; A_rr is real)
 *       A = L L^H once; for every channel c: L y = P_c, L^H G_c = y             (inner sums in "dereverb"'s order)
 *       d^(i)_{t,c} = X_{t,c} - sum_r conj(G_rc) x~_t[r]                        (r ascending over the entries whose frame exists)
 *   output d^(I); optional magnitude M_{t,c} = sqrtf(fmaf(dre, dre, dim * dim))
 * The sums over t run frame after frame from t = 0; phi's per-channel sums are the partial sums of the frames t = q mod LPB, added
 * for q ascending, LPB = 16, 32 or 64 from (C, K) alone.  No order depends on the batch or on which bins share the call.
 * Parameters: adn_wpe_params.  NULL = the defaults of "dereverb" with taps = 32 / C (integer division: 32, 16, 10, 8, 6, 5, 4, 4),
 * the longest filter the stacked size 32 admits -- a design value from the host figures, not tuned by ear.
 * Legal (ADN_ERR_INVALID otherwise, before any launch, the message starts "adn_wpe_mc" and names the field): the ranges of
 * "dereverb", 1 <= channels <= 8 and channels * taps <= 32.
 * Consequences: with C = 1 every statement reduces to "dereverb", and adn_wpe_mc(channels = 1) returns adn_wpe's bits (the call is
 * forwarded to the same kernel); the first D frames of every channel come back bit for bit; a group with T <= D comes back bit
 * for bit; an all-zero group gives zeros; a non-finite value is confined to its own (group, bin), whose content is then
 * unspecified.
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_dereverb_mc.py: per group
 * max |d - d64| <= 4 FLOOR max |d64|, FLOOR the error of the same statements run in fp32 on the host).  Pinned bit for bit: two
 * calls give the same result; a group gives the same bits alone or in any batch; a bin gives the same bits whichever other bins
 * are in the call.  NOT pinned: the bits against numpy; the bits under a permutation of the channels (the stacked order enters
 * every sum).  Deterministic: no atomics.
 *
 * Layouts: spec and spec_out are (n_groups * channels, n_frames, n_bins, 2) fp32, the C channels of a group consecutive clips --
 * what adn_stft_complex writes for an (n_groups * C, L) batch -- 8-byte aligned; they may not overlap.  mag_out may be NULL;
 * otherwise it is (n_groups * channels, 1, n_bins, width) fp32 with width >= n_frames.  The call writes columns [0, n_frames) of
 * mag_out, all of spec_out and not one byte else.  It may use the workspace and only the workspace; adn_wpe_mc_workspace_bytes
 * reports 0 today, and workspace may then be NULL.
 * Cost: one launch for all iterations, n_groups x ceil(n_bins / B) workgroups, B = 16, 8 or 4 bins from (C, K) (B C <= 32); the
 * frames pass through LDS in chunks, so no limit on n_frames comes from LDS.  Per (group, bin) and iteration
 * 4 T (N (N + 1) / 2 + 2 N C) FMAs.  No atomics, no constant table; nothing blocks or allocates.
 * Limits (ADN_ERR_INVALID before any launch): as adn_wpe, with n_groups in n_clips' place, and n_groups * channels < 2^31.
 * ADN_ERR_WORKSPACE: workspace_bytes below adn_wpe_mc_workspace_bytes.  Element offsets are 64-bit.
 * For audio that is still arriving, the recursive joint form: "dereverb stream multichannel", below.
 * Combining the channels into one: "beamform", below.
 * Not here: N > 32; any tuning by ear. */
ADN_API int adn_wpe_mc_workspace_bytes(int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params,
                                       size_t *bytes);
ADN_API int adn_wpe_mc(const float *spec, int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params,
                       void *workspace, size_t workspace_bytes, float *spec_out, float *mag_out, int width, void *stream);

/* ---- dereverb stream: recursive WPE, one update per frame, for audio that is still arriving -----------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement:
 * tests/dereverb_stream_ref.py); it is UNPINNED against any package, like its offline sibling "dereverb".  It is a different
 * algorithm from that one, not a streaming evaluation of it: recursive least squares per (stream, bin) row -- a K x K inverse
 * correlation matrix P and K taps g are carried and updated once per frame, the variance is the a-priori error's own power with a
 * floor that follows the row's running power.  It is causal: d_t depends on X_0 ... X_t only.
 * Not validated: the defaults are the values of the host prototype; they were not tuned by ear.  They differ on purpose from the
 * offline loading and power_floor, whose meanings are different.
 *
 * Every (stream, bin) row is independent.  X_t are the row's complex values, t = 0, 1, ..., and X_t = 0 for t < 0.  In fp32:
 *   first frame (t = 0):  g = 0 (K taps),  P = (1 / delta) I (K x K),  s_0 = p_0
 *   p_t    = fmaf(re, re, im * im)
 *   s_t    = beta s_{t-1} + (1 - beta) p_t                      (t > 0)
 *   phi_t  = max(rho s_t, 1e-30)
 *   x~_j   = X_{t-D-j},  j = 0 ... K-1                          (raw inputs, never outputs)
 *   e_t    = X_t - sum_j conj(g_j) x~_j                         (the a-priori error = the OUTPUT d_t; j ascending)
 *   lam_t  = max(|e_t|^2, phi_t)                                (|.|^2 as p_t)
 *   u_j    = sum_k P_jk x~_k                                    (k ascending)
 *   q      = sum_j Re(conj(x~_j) u_j)                           (j ascending)
 *   den    = alpha lam_t + q
 *   k_j    = u_j / den
 *   P_jk  <- (P_jk - k_j conj(u_k)) / alpha   for j >= k;  Im P_jj := 0;  P_kj := conj(P_jk)
 *   g_j   <- g_j + k_j conj(e_t)
 *   M_t    = sqrtf(fmaf(e.re, e.re, e.im * e.im))               (the optional magnitude)
 * The Hermitian update is part of the DEFINITION: only the lower triangle is computed, the upper one is its conjugate.  The plain
 * update P <- (P - k u^H) / alpha loses the symmetry to rounding and diverges within a few hundred frames, in float64 as well.
 * Arithmetic: a complex multiply-add is two fmaf per component, the real-part product first (acc.re = fmaf(-+a.im b.im,
 * fmaf(a.re, b.re, acc.re)), acc.im = fmaf(a.im b.re, fmaf(+-a.re b.im, acc.im))); the sums of e_t, u_j and q start at +0, and
 * e_t is X_t minus the finished sum; s_t is two products and their sum, den a product and a sum, each rounded; the divisions by
 * den and by alpha are divisions, componentwise and correctly rounded, as is the square root.  max(x, c) is `x < c ? c : x`: a
 * NaN x stays NaN.  1 / delta and 1 - beta are computed once, in fp32.
 * The recursion is exact RLS: with the lam_t it produced, g after T frames solves
 *   (alpha^T delta I + sum_t alpha^(T-1-t) x~_t x~_t^H / lam_t) g = sum_t alpha^(T-1-t) x~_t conj(X_t) / lam_t;
 * with alpha = 1 that is the growing-window solution (tests/test_dereverb_stream_host.py, to 1e-9 in float64).
 * Parameters (adn_wpe_stream_params; NULL = the defaults): taps K 20, delay D 3, forget alpha 0.99, loading delta 300,
 * power_floor rho 0.01, smooth beta 0.9.  delta is dimensionless (x~ x~^H / lam is); it is the inverse of P's first diagonal.
 * Legal (ADN_ERR_INVALID otherwise, before any launch, the message names the field; a NaN is illegal): 1 <= taps <= 32;
 * 1 <= delay <= 8; 0.95 <= forget <= 1; 1 <= loading <= 1e6; 0 < power_floor <= 1; 0 <= smooth < 1.
 * Consequences: the first D frames of a row come back bit for bit (no tap has a frame: e_t = X_t - (+0)); an all-zero row gives
 * zeros; a non-finite value is confined to its own (stream, bin) row, which stays poisoned from then on.
 * Not claimed: a row that is exactly zero for very long with alpha < 1 grows P by 1 / alpha per frame (the wind-up of every
 * exponentially forgetting RLS) and overflows fp32 after about ln(3e38 delta) / -ln(alpha) frames (9400 at the defaults).
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_dereverb_stream.py: per row
 * max |d - d64| <= 4 FLOOR max |d64|, FLOOR the error of the same statements run in fp32 on the host); it is NOT pinned bit for bit
 * to numpy.  Beside that, every (row, bin) is bounded against its own level (tests/recursive_bounds.py):
 * E = max_t |d - d64| / max_t |d64| <= 4 floor.  The floor is the case's own: the largest E of the fp32 restatement on the very
 * spectrogram the device ran on, over every bin of the case's three rows and over two fp32 arithmetics -- every product rounded,
 * and the "Arithmetic" paragraph above followed statement for statement -- measured when the test runs, never below 2^-23, never
 * a device figure and never above 1e-4.  The same bound holds a spectrogram tilted by 80 dB over the bins.  The operator is NOT
 * scale invariant (1 / delta and the 1e-30 under phi_t are absolute), so no power of two is pinned.  Pinned bit for bit: mag_out
 * is sqrtf(fmaf(re, re, im * im)) of the spec_out of the same call; two calls give the same result; cutting a row's frames into
 * calls (the carried state) changes nothing; a row gives the same bits alone or in any batch, in whatever slot; a bin gives the
 * same bits whichever other bins share the call; a stream of the pool equals the same stream in lockstep.  Deterministic: no
 * atomics, no reduction across lanes.
 *
 * State (adn_wpe_stream_state_bytes(n_slots, n_bins, params), caller-owned, opaque, 8-byte aligned, its size depends on taps and
 * delay): per (slot, bin) the taps g, the full P, s, and a ring of the last D + K raw frames indexed by the frame number -- the
 * history lives here, not in a stream's X ring, which is overwritten with d.  A ROW WHOSE FIRST FRAME OF THE CALL IS FRAME 0
 * STARTS FRESH whatever the state holds: there is no reset call, no sentinel and no flag; the state may be handed over holding
 * anything, and a pool slot is reused without a reset.  Any other call continues the row at the frame after its last one; the
 * frames of a row go in order.  The state is read and written by the lanes that own the row.
 *
 * Three entry points, one step function, three places the frames come from:
 *   adn_wpe_online: spec and spec_out are frame-major (n_rows, n_frames, n_bins, 2) fp32 as adn_stft_complex writes it, 8-byte
 *     aligned, and may not overlap; they hold the frames first_frame ... first_frame + n_frames - 1 of every row.  Row i uses slot
 *     i of the state.  mag_out may be NULL; otherwise (n_rows, 1, n_bins, width) fp32, the network-output layout: the call writes
 *     columns [col0, col0 + n_frames) of it, all of spec_out, the state of its rows, and not one byte else.
 *   adn_wpe_stream: between adn_stream_analyze and adn_stream_emit of the same steps (the geometry arguments are theirs; lookahead
 *     must be 0, the operator is causal).  It reads the frames f_first ... f_last the steps emit from the X ring of stream_state,
 *     writes d_t back into the same ring cells, and M_t into columns [window - block, window) of y, the (n_streams * n_steps, 1, F,
 *     window) windows buffer adn_stream_analyze wrote -- no other byte of it, and nothing for the frames at and past the end of a
 *     finished stream.  adn_stream_emit then does what it always does, magnitude from y and phase from the X ring: the inverse STFT
 *     of |d| with the phase of d, the rule Dereverberator uses offline.  Stream i uses slot i of wpe_state (n_streams slots).
 *   adn_wpe_stream_pool: the same between adn_stream_pool_analyze and adn_stream_pool_emit, for their rows (slot, step,
 *     final_length), handed to the kernel by value; y is the (n_rows, 1, F, window) buffer.  wpe_state has n_slots slots.
 * Cost: one launch, n_rows x ceil(n_bins / 8) workgroups of 8 rows; no workspace, no atomics, no constant table (a capture may
 * hold a first call); nothing blocks or allocates.  A call's time is the per-frame chain of a workgroup (measured: 8 us a frame),
 * not the state's bytes (0.17 of their bound at 256 feeds): profiles/bench_dereverb_stream.md.
 * Limits (ADN_ERR_INVALID before any launch): NULL or misaligned pointers; every count >= 1; n_slots, n_bins <= 2^20;
 * first_frame >= 0, first_frame + n_frames < 2^31; n_rows <= n_slots; col0 >= 0 and col0 + n_frames <= width with a mag_out;
 * overlapping spec and spec_out; lookahead != 0; everything adn_stream_emit / adn_stream_pool_emit refuse about the geometry, the
 * steps and the rows (more than ADN_STREAM_POOL_MAX_ROWS rows, a slot out of range or named twice); launch grid < 2^31 workgroups;
 * the parameters as above.  ADN_ERR_WORKSPACE: a state below its size function's bytes.  Element offsets are 64-bit.
 * adn_wpe_stream_state_bytes is host-only (no device needed).
 * More than one channel treated jointly: the next section, "dereverb stream multichannel".
 * Not here: look-ahead or iterated online variants; any tuning by ear. */
typedef struct adn_wpe_stream_params { int taps, delay; float forget, loading, power_floor, smooth; } adn_wpe_stream_params;
ADN_API int adn_wpe_stream_state_bytes(int n_slots, int n_bins, const adn_wpe_stream_params *params, size_t *bytes);
ADN_API int adn_wpe_online(const float *spec, int n_rows, int n_frames, int n_bins, long first_frame,
                           const adn_wpe_stream_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out,
                           float *mag_out, int width, int col0, void *stream);
ADN_API int adn_wpe_stream(void *stream_state, size_t stream_state_bytes, float *y, int n_streams, long first_step, int n_steps,
                           long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                           const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream);
ADN_API int adn_wpe_stream_pool(void *pool_state, size_t pool_state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                                int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                                const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream);

/* ---- dereverb stream multichannel: recursive joint WPE of the channels of a live recording -----------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement:
 * tests/dereverb_mc_stream_ref.py); it is UNPINNED against any package.  It is to "dereverb stream" what "dereverb multichannel" is
 * to "dereverb": recursive least squares per (group, bin), every channel's late reverberation predicted from the past frames of
 * ALL channels of the recording, one variance per frame shared by the channels.  It is causal.
 * Not validated: the defaults are the parent's with the longest filter the stacked size admits; they were not tuned by ear.
 *
 * A group is the C channels of one recording, 1 <= C <= 8, and N = C K <= 32; every (group, bin) is independent.  X_{t,c} is
 * channel c at frame t, zero for t < 0.  The stacked vector is "dereverb multichannel"'s: x~[r] = X_{t-D-j, c} at r = c K + j, from
 * raw inputs, never outputs.  G is N x C (column c predicts channel c), P is N x N.  In fp32, with the rounding rules of "dereverb
 * stream" (a complex multiply-add is two fmaf per component, the real-part product first; sums start at +0; divisions and the
 * square root are correctly rounded, componentwise; max(x, c) is `x < c ? c : x`; 1 / delta and 1 - beta are formed once in fp32):
 *   first frame (t = 0):  G = 0 (N x C),  P = (1 / delta) I (N x N),  s_0 = p_0
 *   p_t    = (sum_c fmaf(re_c, re_c, im_c * im_c)) / C                 (c ascending, then one division by (float) C)
 *   s_t    = beta s_{t-1} + (1 - beta) p_t                              (t > 0)
 *   phi_t  = max(rho s_t, 1e-30)
 *   e_c    = X_{t,c} - sum_r conj(G_rc) x~_r                            (r ascending; the OUTPUT d_{t,c})
 *   lam_t  = max((sum_c |e_c|^2) / C, phi_t)                            (c ascending; |.|^2 as p)
 *   u_r    = sum_s P_rs x~_s   (s ascending);   q = sum_r Re(conj(x~_r) u_r)   (r ascending)
 *   den    = alpha lam_t + q;   k_r = u_r / den
 *   P_rs  <- (P_rs - k_r conj(u_s)) / alpha for r >= s;  Im P_rr := 0;  P_sr := conj(P_rs)
 *   G_rc  <- G_rc + k_r conj(e_c)
 *   M_{t,c} = sqrtf(fmaf(e.re, e.re, e.im * e.im))                      (the optional magnitude)
 * The Hermitian update is part of the DEFINITION, as in "dereverb stream".  The recursion is exact RLS with C right-hand sides:
 * with the lam_t it produced, G after T frames solves the stacked normal equations
 *   (alpha^T delta I + sum_t alpha^(T-1-t) x~_t x~_t^H / lam_t) G_c = sum_t alpha^(T-1-t) x~_t conj(X_{t,c}) / lam_t
 * (tests/test_dereverb_mc_stream_host.py, alpha = 1, to 1e-9 in float64).
 * Parameters: adn_wpe_stream_params, taps PER CHANNEL.  NULL = the defaults of "dereverb stream" with taps = 32 / C (integer
 * division).
 * Legal (ADN_ERR_INVALID otherwise, before any launch, the message starts with the function's name and names the field): the
 * ranges of "dereverb stream"; 1 <= channels <= 8; channels * taps <= 32; and for C >= 2 additionally 2 N (1 - forget) <= 1,
 * evaluated in double on the fp32 value of forget: N = 32 admits forget >= 0.984375, N = 16 0.96875, and N <= 10 every fp32 value
 * above 0.95 (0.95f itself is 0.94999999 and misses the rule at N = 10 by 2.4e-7).  The reason: 1 / (1 - forget) is the length of
 * the window in frames, and below the rule the window holds fewer frames than twice the N unknowns; the fp32 recursion then loses
 * accuracy or goes non-finite at N = 32 -- on the host, 40 s at N = 32: forget 0.985 stays finite (error 5e-4 of the maximum);
 * forget 0.97 reaches 2.4e-3 at (2, 16) and diverges at (8, 4); forget 0.95 goes non-finite at (8, 4) within 30 s, and stays
 * finite at N = 20, 16 and 10 (profiles/bench_dereverb_mc_stream.md).  The rule does not apply to C = 1, whose definition and
 * pins are "dereverb stream"'s.
 * Consequences: with C = 1 every statement is "dereverb stream" ((+0 + p) / 1 = p), the call is forwarded to that kernel and
 * returns its bits, state included; the first D frames of every channel come back bit for bit; an all-zero group gives zeros; a
 * non-finite value is confined to its own (group, bin) -- ALL C channels of that bin stay poisoned from then on, no other bin or
 * group is touched; a group whose first frame of the call is frame 0 starts fresh whatever the state holds: no reset, no
 * sentinel.  Not claimed: the wind-up of an exactly-zero group, as in "dereverb stream".
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_dereverb_mc_stream.py: per group
 * max |d - d64| <= 4 FLOOR max |d64|, FLOOR the error of the same statements run in fp32 on the host).  Beside that, every
 * (channel row, bin) is bounded against its own level, E = max_t |d - d64| / max_t |d64| <= 4 floor, the floor the case's own as in
 * "dereverb stream": over every bin of the case's three groups and both fp32 arithmetics, measured when the test runs on the
 * spectrogram the device ran on, never below 2^-23, never a device figure, never above 1e-4 (tests/recursive_bounds.py); a
 * spectrogram tilted by 80 dB over the bins is held to the same bound, and no power of two is pinned, for the parent's reason.
 * Pinned bit for bit: mag_out is sqrtf(fmaf(re, re, im * im)) of the spec_out of the same call; two
 * calls give the same result; any cut of a group's frames into calls; a group alone or in any batch, in whatever slot; a bin
 * whichever other bins share the call; a lockstep stream (adn_wpe_mc_stream) against adn_wpe_mc_online on the same spectrogram.
 * NOT pinned: the bits against numpy; a permutation of the channels (the stacked order enters every sum).  Deterministic: no
 * atomics, no reduction across lanes.
 *
 * State (adn_wpe_mc_stream_state_bytes(n_slots, channels, n_bins, params), caller-owned, opaque, 8-byte aligned; its size depends
 * on channels, taps and delay; host-only, and it validates everything about the parameters): per (slot, bin) the full P, G, s and
 * per channel a ring of the last D + K raw frames.  A slot is a GROUP.  With channels = 1 it is adn_wpe_stream_state_bytes'.
 *
 * Three entry points, one step function:
 *   adn_wpe_mc_online: adn_wpe_online with the leading dimension n_groups * channels, a group's channels consecutive rows --
 *     adn_wpe_mc's layout; mag_out (n_groups * channels, 1, n_bins, width), columns [col0, col0 + n_frames).  Group i uses slot i.
 *     It writes those columns, all of spec_out, the state of its groups, and not one byte else.
 *   adn_wpe_mc_stream: adn_wpe_stream for an adn_stream_* state whose streams g C ... g C + C - 1 are group g (n_streams a
 *     multiple of channels): d in place into each channel's ring cells, M into columns [window - block, window) of each channel's
 *     windows of y.  wpe_state has n_streams / channels slots.  adn_stream_analyze and adn_stream_emit are what they were.
 *   adn_wpe_mc_stream_pool: adn_wpe_stream_pool for a pool of RECORDINGS, between adn_stream_pool_analyze and
 *     adn_stream_pool_emit on the same rows.  A recording is `channels` consecutive streams of the pool, the same count for the
 *     whole pool (n_slots a multiple of it): recording r owns the stream slots r C ... r C + C - 1 and slot r of wpe_state, which has
 *     n_slots / channels slots.  In the row table a recording is C consecutive rows that name its slots in channel order and carry
 *     the same step and final_length; the recordings of a call come in any order, and n_rows / channels of them fit one call.  It
 *     reads the frames the step emits from the ring cells of the recording's C slots, writes d back into the same cells and M into
 *     columns [window - block, window) of the C rows' windows of y, the (n_rows, 1, F, window) buffer, reads and writes slot r of
 *     wpe_state, and not one byte else: the slots of wpe_state the call does not name keep their bytes.  The table travels by
 *     value; one launch.  Pinned bit for bit: the ring cells, the window columns and the state bytes against adn_wpe_mc_stream on a
 *     lockstep state holding the same rings (tests/test_gpu_stream_pool_mc.py).  With channels = 1 the call is
 *     adn_wpe_stream_pool's kernel and returns its bits, state included.
 * Cost: one launch, n_groups x ceil(n_bins / 8) workgroups of 8 bins, 32 lanes per (group, bin); no workspace, no atomics, no
 * constant table; nothing blocks or allocates.  A call's time is the per-frame chain of a workgroup:
 * profiles/bench_dereverb_mc_stream.md.
 * Limits (ADN_ERR_INVALID before any launch; a refused call writes nothing): those of adn_wpe_online with n_groups in n_rows'
 * place, and n_groups * channels < 2^31; everything adn_wpe_stream refuses, and n_streams % channels != 0; for the pool
 * everything adn_wpe_stream_pool refuses, the parameter rules above, and n_slots % channels != 0, n_rows % channels != 0, a group
 * whose first slot is no multiple of channels, whose slots are not consecutive in channel order, or whose rows differ in step or
 * final_length.  ADN_ERR_WORKSPACE: a state below adn_wpe_mc_stream_state_bytes.  Element offsets are 64-bit.
 * Combining the channels into one: "beamform" (offline) and "beamform stream" (live, on the same stream state) below.
 * Not here: the stream pool with mixed channel counts (one count per pool); more than one step per recording and call; look-ahead;
 * N > 32; any tuning by ear. */
ADN_API int adn_wpe_mc_stream_state_bytes(int n_slots, int channels, int n_bins, const adn_wpe_stream_params *params, size_t *bytes);
ADN_API int adn_wpe_mc_online(const float *spec, int n_groups, int channels, int n_frames, int n_bins, long first_frame,
                              const adn_wpe_stream_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out,
                              float *mag_out, int width, int col0, void *stream);
ADN_API int adn_wpe_mc_stream(void *stream_state, size_t stream_state_bytes, float *y, int n_streams, int channels, long first_step,
                              int n_steps, long final_length, int n_fft, int hop, int window, int block, int lookahead,
                              int max_steps, const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes,
                              void *stream);
ADN_API int adn_wpe_mc_stream_pool(void *pool_state, size_t pool_state_bytes, int n_slots, int channels, int n_fft, int hop,
                                   int window, int block, int lookahead, long ring_samples, const adn_stream_pool_row *rows,
                                   int n_rows, float *y, const adn_wpe_stream_params *params, void *wpe_state,
                                   size_t wpe_state_bytes, void *stream);

/* ---- beamform: mask-driven MVDR, the channels of a recording to one enhanced channel ---------------------------------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement:
 * tests/beamform_ref.py); it is UNPINNED against any package.  It is the MVDR beamformer in Souden's form (Souden, Benesty and
 * Affes 2010), w = Phi_n^-1 Phi_s u / tr(Phi_n^-1 Phi_s), with the two spatial covariance matrices weighted by a time-frequency
 * mask, and the mask taken from ANY per-channel magnitude estimate of the wanted signal: the Wiener gain of "baseline"
 * (adn_spectral_gain), the magnitudes adn_wpe_mc returns, or the U-Net's output -- all three write the layout read here.
 * Not validated: the defaults are the values of the host prototype (profiles/bench_beamform.md); they were not tuned by ear.
 *
 * A group is the C channels of one recording, 1 <= C <= 8; every (group, bin) is independent.  X_{t,c} is the complex STFT of
 * channel c at frame t, M_{t,c} >= 0 the magnitude estimate.  In fp32, with the rounding rules of "dereverb" (the weight applied
 * once as m_t X_{t,r}, each component rounded; complex multiply-adds as two fmaf per component; max(x, c) as `x < c ? c : x` and
 * min(x, c) as `x > c ? c : x`, so a NaN x stays NaN; correctly rounded division and square root; no fp contraction):
 *   p_{t,c} = fmaf(re, re, im * im)
 *   s_t = sum_c M_{t,c}^2,   q_t = sum_c p_{t,c}                               (c ascending from 0; each square rounded, then added)
 *   m_t = q_t > 0 ? min(max(s_t / q_t, rho), 1 - rho) : rho,   n_t = 1 - m_t   (1 - rho rounded once)
 *   Phi_s[r][k] = sum_t (m_t X_{t,r}) conj(X_{t,k}),   Phi_n likewise with n_t (r >= k; the upper triangle is the conjugate and
 *                                                                              the imaginary part of the diagonal is dropped)
 *   A = Phi_n + ((delta tr(Phi_n)) / C + 1e-30) I                              (tr over r ascending; the diagonal is real)
 *   A = L L^H once; for every column c: L y = Phi_s[:, c], L^H G_c = y         (inner sums in "dereverb"'s order)
 *   tau = max(sum_c Re G_cc, 1e-30)                                            (c ascending)
 *   w_c = G[c][ref] / tau                                                      (row c of column ref, each component divided)
 *   Y_t = sum_c conj(w_c) X_{t,c}                                              (c ascending from 0; re: X.x w.x, then X.y w.y;
 *                                                                               im: -X.x w.y, then X.y w.x)
 *   optional M^out_t = sqrtf(fmaf(Yre, Yre, Yim * Yim))
 * The sums over t run frame after frame from t = 0, (m_t X_{t,r}) conj(X_{t,k}) accumulated as re: u.x v.x, then u.y v.y; im:
 * u.y v.x, then -u.x v.y ("dereverb"'s order).  No order depends on the batch or on which bins share the call.  The clip of the
 * mask to [rho, 1 - rho] is part of the definition: it keeps Phi_n from vanishing on a clean recording and Phi_s from vanishing
 * on a noise-only bin, so no input with energy gives a degenerate solve.
 * Parameters (adn_mvdr_params; NULL = the defaults): ref_channel 0, loading delta 1e-3, mask_floor rho 1e-3 -- the values of the
 * host prototype, not tuned by ear.  Legal (ADN_ERR_INVALID otherwise, before any launch, the message starts "adn_mvdr" and names
 * the field; a NaN is illegal): 0 <= ref_channel < channels; 1e-6 <= loading <= 1; 1e-6 <= mask_floor <= 0.25.
 * Consequences: with C = 1, G is real, w = G / G = 1 and the output equals X as values (a signed zero may differ) in every bin whose
 * G is at least 1e-30; an all-zero group gives zeros (A = 1e-30 I, Phi_s = 0, w = 0); a non-finite value is confined to its own
 * (group, bin), whose content is then unspecified.  NOT a consequence: invariance under a common scale of M -- n_t = 1 - m_t does
 * not scale with m_t, so even a power of two changes the result (the restatement confirms that it does).
 *
 * What is pinned.  The result is bounded against the float64 restatement (tests/test_gpu_beamform.py: per group
 * max |Y - Y64| <= 4 FLOOR max |Y64|, FLOOR the error of the same statements run in fp32 on the host).  mag_out is bit for bit
 * sqrtf(fmaf(re, re, im * im)) of spec_out.  Pinned bit for bit: two calls give the same result; a group gives the same bits alone
 * or in any batch; a bin gives the same bits whichever other bins are in the call; mag_width and width do not enter.  NOT pinned: the
 * bits against numpy; the bits under a permutation of the channels.  Deterministic: no atomics.
 *
 * Layouts: spec is (n_groups * channels, n_frames, n_bins, 2) fp32, the C channels of a group consecutive clips -- adn_wpe_mc's
 * layout, what adn_stft_complex writes for an (n_groups * C, L) batch -- 8-byte aligned.  mag is (n_groups * channels, 1, n_bins,
 * mag_width) fp32 with mag_width >= n_frames, columns [0, n_frames) read: what adn_spectral_gain, adn_wpe_mc and the U-Net write.
 * spec_out is (n_groups, n_frames, n_bins, 2), 8-byte aligned.  mag_out may be NULL; otherwise it is (n_groups, 1, n_bins, width)
 * with width >= n_frames, the layout adn_denoise_resynth reads.  No output may overlap an input or the other output.  The call
 * writes columns [0, n_frames) of mag_out, all of spec_out and not one byte else.  It may use the workspace and only the
 * workspace; adn_mvdr_workspace_bytes reports 0 today (the covariances, the factor and the filter stay on chip), and workspace may
 * then be NULL.
 * Cost: one launch, n_groups x ceil(n_bins / B) workgroups of one wave, B = 16 bins up to C = 4 and 8 beyond; the frames pass through LDS in
 * chunks, twice (the sums, then the filter), so no limit on n_frames comes from LDS.  Per (group, bin) 4 T (C (C + 1) + C) FMAs.
 * No atomics, no constant table (a capture may hold a first call); nothing blocks or allocates.
 * Limits (ADN_ERR_INVALID before any launch; a refused call writes nothing): NULL or misaligned spec / mag / spec_out / mag_out;
 * n_groups, n_frames, n_bins >= 1; n_groups * channels < 2^31; mag_width >= n_frames; width >= n_frames with a mag_out; overlap;
 * launch grid < 2^31 workgroups; the parameters as above.  ADN_ERR_WORKSPACE: workspace_bytes below adn_mvdr_workspace_bytes.
 * Element offsets are 64-bit.
 * Not here: streaming or recursive beamforming (that is the next section, "beamform stream"); GEV or rank-one variants; WPD (the
 * joint convolutional beamformer); more than 8 channels; any tuning by ear. */
typedef struct adn_mvdr_params { int ref_channel; float loading, mask_floor; } adn_mvdr_params;
ADN_API int adn_mvdr_workspace_bytes(int n_groups, int channels, int n_frames, int n_bins, const adn_mvdr_params *params,
                                     size_t *bytes);
ADN_API int adn_mvdr(const float *spec, const float *mag, int mag_width, int n_groups, int channels, int n_frames, int n_bins,
                     const adn_mvdr_params *params, void *workspace, size_t workspace_bytes, float *spec_out, float *mag_out,
                     int width, void *stream);

/* ---- beamform stream: recursive covariances, one filter per refresh, for a recording that is still arriving ------------------------
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement:
 * tests/beamform_stream_ref.py); it is UNPINNED against any package.  It is to "beamform" what "dereverb stream multichannel" is
 * to "dereverb multichannel": the two mask-weighted spatial covariances are carried on the device with a forgetting factor, updated
 * once per frame, and the filter of "beamform" is solved from them every R frames.  It is causal.
 * Not validated: forget 0.99 is a window of 100 frames, 1.6 s at hop 128 and 8 kHz -- a design value, not tuned by ear; the other
 * defaults are "beamform"'s.
 *
 * A group is the C channels of one recording, 1 <= C <= 8; every (group, bin) is independent.  In fp32, with the rounding rules of
 * "beamform" (no fp contraction; complex multiply-adds as two fmaf per component in that section's order; max / min that keep a
 * NaN; correctly rounded division and square root):
 *   frame 0 of a group:  Phi_s = Phi_n = +0
 *   m_t, n_t             exactly "beamform"'s, from M_{t,c} and X_{t,c}, rho = mask_floor
 *   for r >= k:          Phi_s[r][k] <- (m_t X_{t,r}) conj(X_{t,k}) + alpha (.) Phi_s[r][k];   Phi_n likewise with n_t
 *   if t % R == 0:       w <- "beamform"'s filter from the current Phi_s, Phi_n: A = Phi_n + ((delta tr Phi_n) / C + 1e-30) I, one
 *                        Cholesky, C columns, tau, w_c = G[c][ref] / tau.  The diagonal's imaginary part is dropped where
 *                        "beamform" drops it -- at use, not in the carried sum
 *   else:                w is the carried one
 *   Y_t = sum_c conj(w_c) X_{t,c}                                              ("beamform"'s order)
 *   optional M^out_t = sqrtf(fmaf(Yre, Yre, Yim * Yim))
 * alpha (.) Phi: each component is multiplied by alpha and rounded once; that product is the addend of the complex multiply-add
 * (re: u.x v.x, then u.y v.y; im: u.y v.x, then -u.x v.y).  With alpha = 1 the sums are therefore "beamform"'s own, bit for bit.
 * Frame 0 always solves, so w is always defined.
 * Parameters (adn_mvdr_stream_params; NULL = the defaults): ref_channel 0, refresh R 1, forget alpha 0.99, loading delta 1e-3,
 * mask_floor rho 1e-3.  Legal (ADN_ERR_INVALID otherwise, before any launch, the message starts with the function's name and
 * names the field; a NaN is illegal): 0 <= ref_channel < channels; 1 <= refresh <= 64; 0.9 <= forget <= 1; 1e-6 <= loading <= 1;
 * 1e-6 <= mask_floor <= 0.25.
 * Consequences: with forget = 1 and refresh = 1, Y_{T-1} equals adn_mvdr's Y_{T-1} on frames 0 ... T-1, bit for bit; with
 * refresh = R the frames t % R == 0 equal the refresh = 1 run; with C = 1 the output equals X as values wherever "beamform" says so
 * (every bin whose G is at least 1e-30); an all-zero group gives zeros; a non-finite value is confined to its own (group, bin),
 * which stays poisoned from then on; a group whose first frame of the call is frame 0 starts fresh whatever the state holds: no
 * reset, no sentinel.  There is no wind-up: the covariances decay, and no inverse is carried that could grow -- an exactly-zero
 * stretch leaves Phi <- alpha Phi and a solve of whatever is left.
 * Quality on the host (tests/test_beamform_stream_host.py, profiles/bench_beamform_stream.md): SI-SDR after the first second, float64
 * restatement, defaults: microphone 0 as recorded 1.50 dB; streaming MVDR 5.08 / 7.59 / 7.22 dB at C = 2 / 4 / 8 (offline MVDR with
 * the same mask 4.61 / 7.72 / 9.09).  Every row beats microphone 0 by more than 1 dB, and every row is asserted.
 *
 * What is pinned.  The result is bounded per (group, bin) against the float64 restatement (tests/test_gpu_beamform_stream.py:
 * E <= 4 floor, the floor the largest E of the fp32 restatement of the same case, never below 2^-23).  Pinned bit for bit: two
 * calls give the same result; any cut of a group's frames into calls; a group alone or in any batch, in whatever slot; a bin
 * whichever other bins share the call; mag_out against sqrtf(fmaf(re, re, im * im)) of spec_out; the last frame against adn_mvdr at
 * forget 1, refresh 1; the frames t % R == 0 against refresh 1; a lockstep stream (adn_mvdr_stream) against adn_mvdr_online on the
 * same ring spectrogram and magnitudes.  NOT pinned: the bits against numpy; a permutation of the channels.  Deterministic: no
 * atomics, no reduction across lanes.
 *
 * State (adn_mvdr_stream_state_bytes(n_slots, channels, n_bins, params), caller-owned, opaque, 8-byte aligned; host-only, and it
 * validates everything about the parameters): per (slot, bin) the two packed lower triangles and w, 2 (C (C + 1) + C) floats,
 * entry-major over the bins of a slot.  A slot is a GROUP.
 *
 * Three entry points, one step function:
 *   adn_mvdr_online: spec (n_groups * channels, n_frames, n_bins, 2), the frames first_frame ... first_frame + n_frames - 1 of
 *     every row, a group's channels consecutive rows; mag (n_groups * channels, 1, n_bins, mag_width), columns [mag_col0, mag_col0 +
 *     n_frames) read; spec_out (n_groups, n_frames, n_bins, 2); mag_out (n_groups, 1, n_bins, width), may be NULL, columns [col0,
 *     col0 + n_frames) written.  Group i uses slot i.  It writes those columns, all of spec_out, the state of its groups, and not
 *     one byte else.  No output may overlap an input, the state or the other output.
 *   adn_mvdr_stream: between adn_stream_analyze and adn_stream_emit, for an adn_stream_* state whose streams g C ... g C + C - 1
 *     are group g (n_streams a multiple of channels; lookahead must be 0).  It reads X_{t,c} from every channel's ring cells and
 *     M_{t,c} from columns [window - block, window) of every channel's windows in y -- where adn_spectral_gain_windows or
 *     adn_wpe_mc_stream left it -- and writes Y_t into the ring cells and |Y_t| into the same columns of the windows of the
 *     group's FIRST stream only (g C, whatever ref_channel is), and no other byte; nothing for frames at and past the end of a
 *     finished stream.  The lanes that read a (group, bin, frame) are the ones that write it, so doing this in place is safe.
 *     mvdr_state has n_streams / channels slots.  adn_stream_emit is unchanged: it then emits all streams, and the host keeps row
 *     g C of each group; what the C - 1 unused rows cost is measured in profiles/bench_beamform_stream.md.
 *   adn_mvdr_stream_pool: the same for a pool of RECORDINGS, between adn_stream_pool_analyze and adn_stream_pool_emit; the
 *     recordings, their slots and their rows are adn_wpe_mc_stream_pool's ("dereverb stream multichannel"): recording r owns the
 *     stream slots r C ... r C + C - 1 and slot r of mvdr_state (n_slots / channels slots), and is C consecutive rows in channel
 *     order with one step and final_length.  It reads X_{t,c} from the ring cells of the C slots and M_{t,c} from columns
 *     [window - block, window) of the C rows' windows of y, the (n_rows, 1, F, window) buffer, and writes Y_t into the ring cells of
 *     the recording's FIRST slot and |Y_t| into the same columns of the group's FIRST row, slot r of mvdr_state, and not one byte
 *     else.  The table travels by value; one launch.  Pinned bit for bit against adn_mvdr_stream on a lockstep state holding the
 *     same rings: ring cells, window columns, state bytes (tests/test_gpu_stream_pool_mc.py).
 *     The emit may then skip the unused channels: adn_stream_pool_emit takes a row table, so the caller hands it the first row of
 *     each group and the first window of each group (y[::C], compacted) and nothing else.  That is safe because the emit kernel
 *     writes no state but a slot's own overlap-add tail, and nothing reads that tail but that slot's own later emits: the slots
 *     r C + 1 ... r C + C - 1 are never emitted, so their tails are never read.
 * Cost: one launch, n_groups x ceil(n_bins / B) workgroups of one wave, B = 16 bins up to C = 4 and 8 beyond; the covariances stay in
 * registers for the whole call; no workspace, no atomics, no constant table (a capture may hold a first call); nothing blocks or
 * allocates.  A call's time is the per-frame chain of a workgroup: profiles/bench_beamform_stream.md.
 * Limits (ADN_ERR_INVALID before any launch; a refused call writes nothing): those of adn_wpe_mc_online and adn_wpe_mc_stream with
 * the new arguments: NULL or misaligned mag; mag_col0 >= 0 and mag_col0 + n_frames <= mag_width; overlap; for the pool what
 * adn_wpe_mc_stream_pool refuses about the pool, the rows and the groups.  ADN_ERR_WORKSPACE: a state below
 * adn_mvdr_stream_state_bytes.  Element offsets are 64-bit.
 * Not here: the stream pool with mixed channel counts; more than one step per recording and call; GEV, rank-one or WPD variants; look-ahead;
 * a lockstep emit that skips the unused channels (adn_stream_emit emits every stream); any tuning by ear. */
typedef struct adn_mvdr_stream_params { int ref_channel, refresh; float forget, loading, mask_floor; } adn_mvdr_stream_params;
ADN_API int adn_mvdr_stream_state_bytes(int n_slots, int channels, int n_bins, const adn_mvdr_stream_params *params, size_t *bytes);
ADN_API int adn_mvdr_online(const float *spec, const float *mag, int mag_width, int mag_col0, int n_groups, int channels,
                            int n_frames, int n_bins, long first_frame, const adn_mvdr_stream_params *params, void *state,
                            size_t state_bytes, int n_slots, float *spec_out, float *mag_out, int width, int col0, void *stream);
ADN_API int adn_mvdr_stream(void *stream_state, size_t stream_state_bytes, float *y, int n_streams, int channels, long first_step,
                            int n_steps, long final_length, int n_fft, int hop, int window, int block, int lookahead,
                            int max_steps, const adn_mvdr_stream_params *params, void *mvdr_state, size_t mvdr_state_bytes,
                            void *stream);
ADN_API int adn_mvdr_stream_pool(void *pool_state, size_t pool_state_bytes, int n_slots, int channels, int n_fft, int hop, int window,
                                 int block, int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                                 const adn_mvdr_stream_params *params, void *mvdr_state, size_t mvdr_state_bytes, void *stream);

/* ---- echo stream: acoustic echo cancellation lives in a header and a library of its own: adn_echo.h and libadn_echo.so.  The symbol
 * table of libadn.so is this header's, name for name, and stays so.  Operators of a two-way call that neither closed table can take
 * -- the pool form of the echo canceller first -- are declared in adn_call.h and exported by libadn_call.so, whose table is open. */

/* ---- environment switches -------------------------------------------------------------------------------------------------
 * Read ONCE, when a U-Net handle is created (never per call).  None is needed in production: the defaults are the measured best
 * and every family below is covered by the parity tests (tests/test_gpu_variants.py::MODES).  They select between kernel
 * families that all compute the reference's forward within the stated tolerance:
 *
 *   ADN_CONV_ALGO=direct     fp32 3x3 layers on the direct implicit-GEMM kernels (conv_mfma) instead of Winograd
 *   ADN_WINO_TILE=2 | 4      fp32: F(2x2,3x3) for every 3x3 layer | F(4x4,3x3) for every plain / pooled 3x3 layer whatever its size
 *   ADN_WINO_SPLITK=1        fp32: split-K wherever the F(2x2,3x3) grid cannot fill the chip (default: only by the small-grid rule)
 *   ADN_BATCH_INVARIANT=1    initial value of adn_unet_set_batch_invariant (above)
 *   ADN_AUTO_GRID=n, ADN_AUTO_GRID64=n   thresholds of the small-grid rule in F(4x4,3x3) workgroups (192 / 512; tools/small_grid_probe.py)
 *   ADN_CONVT_SPLIT=0        fp32 transposed convolutions on the exact-fp32 MFMA instead of the three-term bf16 split
 *   ADN_WINO_GEMM=0 | 2      fp32 3x3 layers at the two deepest levels as input transform + 36 split-bf16 GEMMs + output transform
 *                            (csrc/wino3s_kernels.hip): never | wherever its buffers fit the workspace (default 1: where they fit
 *                            and the GEMM launch fills the chip, or the handle is pinned)
 *   ADN_SPLIT_BN=128 | 256 | 256w8   the GEMM stage of that form on workgroup tiles of 128 rows x 128 columns | x 256 columns, 4 waves |
 *                            x 256 columns, 8 waves, for every layer with Cout % 256 == 0 (default: per layer, as measured;
 *                            bit-identical results; another value is refused when the handle is created)
 *   ADN_F16_CONV=32         fp16 3x3 layers on conv_dma<_Float16> (32x32x16 MFMA) instead of conv16_f16 (16x16x32)
 *   ADN_F16_FIRST=0          fp16: Conv2d(1 -> 64) as its own launch instead of fused into down1's second convolution
 *   ADN_F16_CONVT=dma        fp16 transposed convolutions on conv_dma<_Float16> (32x32x16 MFMA, LDS-staged stores) instead of convt16_f16
 *
 * The library reads no other environment variable; its sources contain no timing-experiment code. */

#ifdef __cplusplus
}
#endif
#endif /* ADN_H */
