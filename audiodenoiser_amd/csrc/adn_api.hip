// C ABI of libadn.so (include/adn.h) outside the U-Net (unet.hip): version, last error, device queries and the argument checks in
// front of the STFT, loader, loss, Griffin-Lim, resampler, mixer, reverb, quality-metric, long-form and streaming denoising launchers.
#include <algorithm>
#include "adn_host.h"

#include <cmath>
#include <string>

using adn::aligned_to;
using adn::DeviceGuard;
using adn::fail;
using adn::fail_hip;
using adn::fail_launch;

thread_local std::string adn::g_err;

extern "C" {

int adn_version(void) { return 1; }

const char *adn_last_error(void) { return adn::g_err.c_str(); }

int adn_device_count(int *count)
{
    if (!count) return fail(ADN_ERR_INVALID, "adn_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail_hip(e, "hipGetDeviceCount");
    }
    *count = n;
    return ADN_OK;
}

int adn_prepare(int device, int n_fft)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ADN_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(ADN_ERR_INVALID, "adn_prepare: bad device index");
    if (n_fft != 0 && (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1))))
        return fail(ADN_ERR_INVALID, "adn_prepare: n_fft must be 0 (loss tables only) or a power of two in [64, 4096]");
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");
    if (n_fft) {
        const float *tables = nullptr;
        ADN_LAUNCH(adn::stft_tables(n_fft, &tables, nullptr), "adn_prepare");
    }
    ADN_LAUNCH(adn::loss_tables(nullptr), "adn_prepare");
    return ADN_OK;
}

int adn_stft_n_frames(long length, int n_fft, int hop, int center, long *n_frames)
{
    if (!n_frames || n_fft < 2 || hop < 1 || length < 0) return fail(ADN_ERR_INVALID, "adn_stft_n_frames: bad argument");
    const long lp = center ? length + 2L * (n_fft / 2) : length;
    *n_frames = lp < n_fft ? 0 : 1 + (lp - n_fft) / hop;
    return ADN_OK;
}

int adn_stft_mag(const float *audio, int n_clips, long length, int n_fft, int hop, int center, float *out, void *stream)
{
    if (!audio || !out) return fail(ADN_ERR_INVALID, "adn_stft_mag: null pointer");
    if (n_clips < 1 || hop < 1) return fail(ADN_ERR_INVALID, "adn_stft_mag: n_clips and hop must be >= 1");
    if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return fail(ADN_ERR_INVALID, "adn_stft_mag: n_fft must be a power of two in [64, 4096]");
    if (length >= (1L << 30) || hop > (1 << 20))
        return fail(ADN_ERR_INVALID, "adn_stft_mag: clip length must be < 2^30 samples and hop <= 2^20");
    long nfr = 0;
    adn_stft_n_frames(length, n_fft, hop, center, &nfr);
    if (nfr <= 0) return fail(ADN_ERR_INVALID, "adn_stft_mag: audio shorter than n_fft");
    const int nb = n_fft / 2 + 1;
    hipError_t e = adn::launch_stft_mag(audio, n_clips, length, n_fft, hop, center, nfr, out, nb, nfr, (long)nb * nfr, 0,
                                        static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stft_mag: hop too large for on-chip staging or grid too large");
    if (e != hipSuccess) return fail_launch(e, "adn_stft_mag");
    return ADN_OK;
}

int adn_stft_mag_fit(const float *audio, int n_clips, long length, int n_fft, int hop, int center, float *out, int H, int W,
                     void *stream)
{
    if (!audio || !out) return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: null pointer");
    if (n_clips < 1 || hop < 1 || H < 1 || W < 1) return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: n_clips, hop, H, W must be >= 1");
    if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: n_fft must be a power of two in [64, 4096]");
    if (length >= (1L << 30) || hop > (1 << 20) || (long)H * W >= (1L << 30))
        return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: clip length and H*W must be < 2^30, hop <= 2^20");
    long nfr = 0;
    adn_stft_n_frames(length, n_fft, hop, center, &nfr);
    if (nfr <= 0) return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: audio shorter than n_fft");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = n_fft / 2 + 1;
    {   // nothing is enqueued when the launch below is going to be refused (cold tables on a capturing stream)
        const float *tables = nullptr;
        ADN_LAUNCH(adn::stft_tables(n_fft, &tables, st), "adn_stft_mag_fit");
    }
    // zero padding at the bottom / right of the window (data_loader.py:59-70) where the spectrogram is smaller than it
    if (W > nfr || H > nb) ADN_HIP(hipMemsetAsync(out, 0, (size_t)n_clips * H * W * sizeof(float), st));
    const long nfc = nfr < W ? nfr : W;                   // frames that fall inside the window: the only ones computed
    hipError_t e = adn::launch_stft_mag(audio, n_clips, length, n_fft, hop, center, nfc, out, nb < H ? nb : H, W, (long)H * W, 1, st);
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stft_mag_fit: hop too large for on-chip staging or grid too large");
    if (e != hipSuccess) return fail_launch(e, "adn_stft_mag_fit");
    return ADN_OK;
}

int adn_quantize_pad(const float *in, int n, int h, int w, float *out, int H, int W, void *stream)
{
    if (!in || !out || n < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(ADN_ERR_INVALID, "adn_quantize_pad: bad argument");
    ADN_HIP(adn::launch_quantize_pad(in, n, h, w, out, H, W, static_cast<hipStream_t>(stream)));
    return ADN_OK;
}

int adn_per_clip_l1(const float *a, const float *b, int n_clips, long elems_per_clip, float *out, void *stream)
{
    if (!a || !b || !out || n_clips < 1 || elems_per_clip < 1) return fail(ADN_ERR_INVALID, "adn_per_clip_l1: bad argument");
    ADN_HIP(adn::launch_per_clip_l1(a, b, n_clips, elems_per_clip, out, static_cast<hipStream_t>(stream)));
    return ADN_OK;
}

int adn_resample_length(long length, int src_rate, int dst_rate, long *out_length)
{
    int up = 0, down = 0;
    if (!out_length) return fail(ADN_ERR_INVALID, "adn_resample_length: null pointer");
    if (!adn::resample_ratio(src_rate, dst_rate, &up, &down))
        return fail(ADN_ERR_INVALID, "adn_resample_length: rates must be >= 1 with max(up, down) <= 4096 after dividing by their gcd");
    if (length < 1) return fail(ADN_ERR_INVALID, "adn_resample_length: length must be >= 1");
    if (length > (0x7fffffffL * down) / up) return fail(ADN_ERR_INVALID, "adn_resample_length: output length must be < 2^31");
    const long m = (length * up + down - 1) / down;
    if (m >= (1L << 31)) return fail(ADN_ERR_INVALID, "adn_resample_length: output length must be < 2^31");
    *out_length = m;
    return ADN_OK;
}

int adn_resample_prepare(int device, int src_rate, int dst_rate)
{
    int up = 0, down = 0;
    if (!adn::resample_ratio(src_rate, dst_rate, &up, &down))
        return fail(ADN_ERR_INVALID, "adn_resample_prepare: rates must be >= 1 with max(up, down) <= 4096 after dividing by their gcd");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ADN_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(ADN_ERR_INVALID, "adn_resample_prepare: bad device index");
    if (up == down) return ADN_OK;                        // equal rates: a copy, no table
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");
    ADN_HIP(adn::resample_prepare(up, down, nullptr));
    adn::ResampleStreamGeom g;                            // ... and adn_resample_stream's, where the pair can be streamed
    if (adn::resample_stream_geom(src_rate, dst_rate, &g) && g.H <= adn::ADN_RESAMPLE_STREAM_MAX_H)
        ADN_HIP(adn::resample_stream_prepare(g, nullptr));
    return ADN_OK;
}

int adn_resample(const float *audio, int n_clips, long length, int src_rate, int dst_rate, float *out, void *stream)
{
    if (!audio || !out) return fail(ADN_ERR_INVALID, "adn_resample: null pointer");
    if (audio == out) return fail(ADN_ERR_INVALID, "adn_resample: out may not alias audio");
    if (n_clips < 1) return fail(ADN_ERR_INVALID, "adn_resample: n_clips must be >= 1");
    long m = 0;
    if (adn_resample_length(length, src_rate, dst_rate, &m) != ADN_OK) return ADN_ERR_INVALID;
    int up = 0, down = 0;
    adn::resample_ratio(src_rate, dst_rate, &up, &down);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (up == down) {
        ADN_HIP(hipMemcpyAsync(out, audio, (size_t)n_clips * length * sizeof(float), hipMemcpyDeviceToDevice, st));
        return ADN_OK;
    }
    hipError_t e = adn::launch_resample(audio, n_clips, length, m, up, down, out, st);
    if (e == adn::ADN_COLD_IN_CAPTURE)
        return fail(ADN_ERR_INVALID, "adn_resample: first use of this (device, rate pair) on a stream that is being captured -- the "
                    "coefficient table is built with a blocking upload; call adn_resample_prepare(device, src_rate, dst_rate) before "
                    "the capture");
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_resample: grid too large (n_clips x output blocks >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, "adn_resample");
    return ADN_OK;
}

int adn_mix_snr_workspace_bytes(int n_clips, long length, size_t *bytes)
{
    if (!bytes || n_clips < 1 || length < 1 || length >= (1L << 40))
        return fail(ADN_ERR_INVALID, "adn_mix_snr_workspace_bytes: need n_clips >= 1 and 1 <= length < 2^40");
    *bytes = adn::mix_snr_workspace_floats(n_clips, length) * sizeof(float);
    return ADN_OK;
}

int adn_mix_snr(const float *clean, const float *noise, int n_clips, long length, float snr_db, void *workspace,
                size_t workspace_bytes, float *out, void *stream)
{
    if (!clean || !noise || !out) return fail(ADN_ERR_INVALID, "adn_mix_snr: null pointer");
    if (out == clean) return fail(ADN_ERR_INVALID, "adn_mix_snr: out may alias noise but not clean");
    size_t need = 0;
    if (adn_mix_snr_workspace_bytes(n_clips, length, &need) != ADN_OK) return ADN_ERR_INVALID;
    if (!(snr_db >= -200.f && snr_db <= 200.f)) return fail(ADN_ERR_INVALID, "adn_mix_snr: snr_db must be in [-200, 200]");
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_mix_snr: workspace too small");
    const float inv_lin = (float)std::pow(10.0, -(double)snr_db / 20.0);
    hipError_t e = adn::launch_mix_snr(clean, noise, n_clips, length, inv_lin, static_cast<float *>(workspace), out,
                                       static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_mix_snr: grid too large (n_clips x length / 8192 >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, "adn_mix_snr");
    return ADN_OK;
}

int adn_reverb(const float *audio, int n_clips, long length, int sample_rate, float room_size, float damping, float wet_level,
               float dry_level, float width, int clip, float *out, void *stream)
{
    if (!audio || !out) return fail(ADN_ERR_INVALID, "adn_reverb: null pointer");
    if (n_clips < 1) return fail(ADN_ERR_INVALID, "adn_reverb: n_clips must be >= 1");
    if (length < 1 || length >= (1L << 30)) return fail(ADN_ERR_INVALID, "adn_reverb: need 1 <= length < 2^30");
    if (!adn::reverb_rate_ok(sample_rate))
        return fail(ADN_ERR_INVALID, "adn_reverb: sample_rate must be in [2000, 128000] (the delay lines of a clip are held in LDS)");
    const float par[5] = {room_size, damping, wet_level, dry_level, width};
    for (float v : par)
        if (!(v >= 0.f && v <= 1.f))
            return fail(ADN_ERR_INVALID, "adn_reverb: room_size, damping, wet_level, dry_level and width must be in [0, 1]");
    // the scalars of adn.h, each operation rounded to fp32 (volatile: no contraction into an fma)
    volatile float t = room_size * 0.28f;
    const float feedback = t + 0.7f;
    const float damp = damping * 0.4f;
    t = wet_level * 3.f;
    t = 0.5f * t;
    volatile float w1 = 1.f + width;
    const float wet1 = t * w1;
    const float dry = dry_level * 2.f;
    hipError_t e = adn::launch_reverb(audio, n_clips, (int)length, sample_rate, feedback, damp, wet1, dry, clip != 0, out,
                                      static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_reverb: unsupported sample_rate");
    if (e != hipSuccess) return fail_hip(e, "adn_reverb");
    return ADN_OK;
}

int adn_quality_workspace_bytes(int n_clips, long length, size_t *bytes)
{
    if (!bytes || n_clips < 1 || length < 1 || length >= adn::ADN_QUALITY_MAX_LENGTH)
        return fail(ADN_ERR_INVALID, "adn_quality_workspace_bytes: need n_clips >= 1 and 1 <= length < 2^30");
    *bytes = adn::quality_workspace_bytes(n_clips, length);
    return ADN_OK;
}

int adn_quality(const float *est, const float *ref, const long *lengths, int n_clips, long length, int seg_frame, void *workspace,
                size_t workspace_bytes, float *out, void *stream)
{
    if (!est || !ref || !out) return fail(ADN_ERR_INVALID, "adn_quality: null pointer");
    size_t need = 0;
    if (adn_quality_workspace_bytes(n_clips, length, &need) != ADN_OK) return ADN_ERR_INVALID;
    if (seg_frame < adn::ADN_SEG_FRAME_MIN || seg_frame > adn::ADN_SEG_FRAME_MAX)
        return fail(ADN_ERR_INVALID, "adn_quality: seg_frame must be in [16, 8192]");
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_quality: workspace too small");
    if (!aligned_to(workspace, 16)) return fail(ADN_ERR_INVALID, "adn_quality: workspace must be 16-byte aligned");
    hipError_t e = adn::launch_quality(est, ref, lengths, n_clips, length, seg_frame, workspace, out, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_quality: grid too large (n_clips x length / 8192 >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, "adn_quality");
    return ADN_OK;
}

int adn_stoi_workspace_bytes(int n_clips, long length, size_t *bytes)
{
    if (!bytes || n_clips < 1 || length < 1 || length >= adn::ADN_QUALITY_MAX_LENGTH)
        return fail(ADN_ERR_INVALID, "adn_stoi_workspace_bytes: need n_clips >= 1 and 1 <= length < 2^30");
    *bytes = adn::stoi_plan(n_clips, length).total;
    return ADN_OK;
}

int adn_stoi(const float *est, const float *ref, const long *lengths, int n_clips, long length, void *workspace,
             size_t workspace_bytes, float *out, void *stream)
{
    if (!est || !ref || !out) return fail(ADN_ERR_INVALID, "adn_stoi: null pointer");
    size_t need = 0;
    if (adn_stoi_workspace_bytes(n_clips, length, &need) != ADN_OK) return ADN_ERR_INVALID;
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_stoi: workspace too small");
    if (!aligned_to(workspace, 16)) return fail(ADN_ERR_INVALID, "adn_stoi: workspace must be 16-byte aligned");
    hipError_t e = adn::launch_stoi(est, ref, lengths, n_clips, length, workspace, out, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stoi: grid too large (n_clips x frames / 64 >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, "adn_stoi");
    return ADN_OK;
}

int adn_perceptual_loss_workspace_bytes(int n_clips, int F, int T, size_t *bytes)
{
    if (!bytes || n_clips < 1 || F < 1 || T < adn::ADN_LOSS_MIN_T || T > adn::ADN_LOSS_MAX_T)
        return fail(ADN_ERR_INVALID, "adn_perceptual_loss_workspace_bytes: need n_clips,F >= 1 and 32 <= T < 2^24");
    *bytes = adn::perceptual_loss_workspace_floats(n_clips, F, T) * sizeof(float);
    return ADN_OK;
}

int adn_perceptual_loss(const float *pred, const float *target, int n_clips, int F, int T, void *workspace,
                        size_t workspace_bytes, float *out, void *stream)
{
    if (!pred || !target || !out) return fail(ADN_ERR_INVALID, "adn_perceptual_loss: null pointer");
    // T >= 32: the mel term's reflect padding of n_fft / 2 = 31 samples needs a longer series (torch.stft / torchaudio raise
    // below that too: loss.py:39-41 with pad_mode "reflect")
    if (n_clips < 1 || F < 1 || T < adn::ADN_LOSS_MIN_T || T > adn::ADN_LOSS_MAX_T ||
        adn::perceptual_loss_lds_bytes(T) > adn::ADN_LOSS_MAX_LDS)
        return fail(ADN_ERR_INVALID, "adn_perceptual_loss: need n_clips,F >= 1 and 32 <= T < 2^24 (reflect padding of the mel "
                                     "term needs T > 31)");
    const size_t need = adn::perceptual_loss_workspace_floats(n_clips, F, T) * sizeof(float);
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_perceptual_loss: workspace too small");
    ADN_LAUNCH(adn::launch_perceptual_loss(pred, target, n_clips, F, T, static_cast<float *>(workspace), out,
                                           static_cast<hipStream_t>(stream)), "adn_perceptual_loss");
    return ADN_OK;
}

int adn_perceptual_loss_backward_workspace_bytes(int n_clips, int F, int T, size_t *bytes)
{
    if (!bytes || n_clips < 1 || F < 1 || T < adn::ADN_LOSS_MIN_T || T > adn::ADN_LOSS_MAX_T)
        return fail(ADN_ERR_INVALID, "adn_perceptual_loss_backward_workspace_bytes: need n_clips,F >= 1 and 32 <= T < 2^24");
    *bytes = adn::perceptual_loss_backward_workspace_floats(n_clips, F, T) * sizeof(float);
    return ADN_OK;
}

int adn_perceptual_loss_backward(const float *pred, const float *target, int n_clips, int F, int T, const float *grad_out,
                                 void *workspace, size_t workspace_bytes, float *grad_pred, float *grad_target, void *stream)
{
    if (!pred || !target || !grad_out) return fail(ADN_ERR_INVALID, "adn_perceptual_loss_backward: null pointer");
    if (!grad_pred && !grad_target)
        return fail(ADN_ERR_INVALID, "adn_perceptual_loss_backward: grad_pred and grad_target are both null");
    if (n_clips < 1 || F < 1 || T < adn::ADN_LOSS_MIN_T || T > adn::ADN_LOSS_MAX_T)
        return fail(ADN_ERR_INVALID, "adn_perceptual_loss_backward: need n_clips,F >= 1 and 32 <= T < 2^24 (reflect padding of "
                                     "the mel term needs T > 31)");
    const size_t need = adn::perceptual_loss_backward_workspace_floats(n_clips, F, T) * sizeof(float);
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_perceptual_loss_backward: workspace too small");
    if (!aligned_to(workspace, 16)) return fail(ADN_ERR_INVALID, "adn_perceptual_loss_backward: workspace must be 16-byte aligned");
    ADN_LAUNCH(adn::launch_perceptual_loss_backward(pred, target, n_clips, F, T, grad_out, static_cast<float *>(workspace),
                                                    grad_pred, grad_target, static_cast<hipStream_t>(stream)),
               "adn_perceptual_loss_backward");
    return ADN_OK;
}

/* ---- inverse STFT / Griffin-Lim (test.py:29-48) -------------------------------------------------------------- */
static bool gl_size_ok(int n_fft) { return n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0; }

int adn_istft_length(int n_frames, int hop, long *length)
{
    if (!length || n_frames < 1 || hop < 1) return fail(ADN_ERR_INVALID, "adn_istft_length: need n_frames, hop >= 1");
    *length = (long)hop * (n_frames - 1);
    return ADN_OK;
}

int adn_stft_complex(const float *audio, int n_clips, long length, int n_fft, int hop, float *spec_out, void *stream)
{
    if (!audio || !spec_out) return fail(ADN_ERR_INVALID, "adn_stft_complex: null pointer");
    if (!gl_size_ok(n_fft)) return fail(ADN_ERR_INVALID, "adn_stft_complex: n_fft must be a power of two in [64, 4096]");
    if (n_clips < 1 || hop < 1 || length < 1 || length >= (1L << 30)) return fail(ADN_ERR_INVALID, "adn_stft_complex: bad sizes");
    const long T = 1 + length / hop;
    if (T > 0x7fffffffL) return fail(ADN_ERR_INVALID, "adn_stft_complex: too many frames");
    if (!aligned_to(spec_out, 8)) return fail(ADN_ERR_INVALID, "adn_stft_complex: spec_out must be 8-byte aligned");
    ADN_LAUNCH(adn::launch_stft_complex(audio, n_clips, length, n_fft, hop, (int)T, spec_out, static_cast<hipStream_t>(stream)),
               "adn_stft_complex");
    return ADN_OK;
}

int adn_istft_workspace_bytes(int n_clips, int n_frames, int n_fft, size_t *bytes)
{
    if (!bytes || n_clips < 1 || n_frames < 2 || !gl_size_ok(n_fft)) return fail(ADN_ERR_INVALID, "adn_istft_workspace_bytes: bad sizes");
    *bytes = (size_t)n_clips * n_frames * n_fft * sizeof(float);
    return ADN_OK;
}

int adn_istft(const float *spec, int n_clips, int n_frames, int n_fft, int hop, void *workspace, size_t workspace_bytes,
              float *audio_out, void *stream)
{
    if (!spec || !audio_out) return fail(ADN_ERR_INVALID, "adn_istft: null pointer");
    if (!gl_size_ok(n_fft) || n_clips < 1 || n_frames < 2 || hop < 1 || hop > n_fft)
        return fail(ADN_ERR_INVALID, "adn_istft: need power-of-two n_fft in [64,4096], n_frames >= 2, 1 <= hop <= n_fft");
    const size_t need = (size_t)n_clips * n_frames * n_fft * sizeof(float);
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_istft: workspace too small");
    if (!aligned_to(spec, 8) || !aligned_to(workspace, 8)) return fail(ADN_ERR_INVALID, "adn_istft: spec and workspace must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ADN_LAUNCH(adn::launch_istft_frames(spec, n_clips, n_frames, n_fft, static_cast<float *>(workspace), st), "adn_istft");
    ADN_HIP(adn::launch_istft_ola(static_cast<const float *>(workspace), n_clips, n_frames, n_fft, hop, audio_out, st));
    return ADN_OK;
}

int adn_griffin_lim_workspace_bytes(int n_clips, int n_bins, int n_frames, size_t *bytes)
{
    if (!bytes || n_clips < 1 || n_bins < 33 || n_frames < 2) return fail(ADN_ERR_INVALID, "adn_griffin_lim_workspace_bytes: bad sizes");
    const size_t n_fft = 2 * (size_t)(n_bins - 1);
    *bytes = (size_t)n_clips * n_frames * ((size_t)n_bins * 2 + n_fft) * sizeof(float);
    return ADN_OK;
}

int adn_griffin_lim(const float *magnitude, const float *rnd, int n_clips, int n_bins, int n_frames, int n_fft, int hop,
                    int iterations, void *workspace, size_t workspace_bytes, float *audio_out, void *stream)
{
    if (!magnitude || !rnd || !audio_out) return fail(ADN_ERR_INVALID, "adn_griffin_lim: null pointer");
    if (!gl_size_ok(n_fft) || n_bins != n_fft / 2 + 1)
        return fail(ADN_ERR_INVALID, "adn_griffin_lim: need power-of-two n_fft in [64,4096] and n_bins = n_fft/2+1");
    if (n_clips < 1 || n_frames < 2 || hop < 1 || hop > n_fft || iterations < 0)
        return fail(ADN_ERR_INVALID, "adn_griffin_lim: need n_clips >= 1, n_frames >= 2, 1 <= hop <= n_fft, iterations >= 0");
    size_t need = 0;
    adn_griffin_lim_workspace_bytes(n_clips, n_bins, n_frames, &need);
    if (!workspace || workspace_bytes < need) return fail(ADN_ERR_WORKSPACE, "adn_griffin_lim: workspace too small");
    if (!aligned_to(workspace, 8)) return fail(ADN_ERR_INVALID, "adn_griffin_lim: workspace must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *spec = static_cast<float *>(workspace);
    float *buf = spec + (size_t)n_clips * n_frames * n_bins * 2;
    const long len = (long)hop * (n_frames - 1);
    {
        const float *tables = nullptr;
        ADN_LAUNCH(adn::stft_tables(n_fft, &tables, st), "adn_griffin_lim");
    }
    ADN_HIP(adn::launch_gl_polar(magnitude, rnd, n_clips, n_bins, n_frames, spec, st));
    for (int it = 0; it <= iterations; ++it) {
        ADN_HIP(adn::launch_istft_frames(spec, n_clips, n_frames, n_fft, buf, st));
        ADN_HIP(adn::launch_istft_ola(buf, n_clips, n_frames, n_fft, hop, audio_out, st));
        if (it < iterations)   // test.py:41-46: S = |Z| exp(i angle Z) with Z = stft(audio) -- Z itself up to rounding
            ADN_HIP(adn::launch_stft_complex(audio_out, n_clips, len, n_fft, hop, n_frames, spec, st));
    }
    return ADN_OK;
}

/* ---- long-form denoising: windows, stitch, resynthesis (adn.h, "denoise") --------------------------------------- */
// element counts are indexed with `long` in the kernels; what is refused is what would not fit the 32-bit frame / grid arithmetic
static const char *denoise_plan_text = ": need n_frames >= 1, window >= 16 and 0 <= overlap <= window / 2";

int adn_denoise_plan(int n_frames, int window, int overlap, int *n_windows, int *window_width)
{
    if (!n_windows || !window_width) return fail(ADN_ERR_INVALID, "adn_denoise_plan: null pointer");
    adn::DenoiseGeom g;
    if (!adn::denoise_geom(n_frames, window, overlap, &g)) return fail(ADN_ERR_INVALID, std::string("adn_denoise_plan") + denoise_plan_text);
    *n_windows = g.K;
    *window_width = g.Wd;
    return ADN_OK;
}

int adn_denoise_windows(const float *spec, int n_clips, int n_frames, int n_bins, int window, int overlap, float *out, void *stream)
{
    if (!spec || !out) return fail(ADN_ERR_INVALID, "adn_denoise_windows: null pointer");
    if (n_clips < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, "adn_denoise_windows: n_clips and n_bins must be >= 1");
    adn::DenoiseGeom g;
    if (!adn::denoise_geom(n_frames, window, overlap, &g)) return fail(ADN_ERR_INVALID, std::string("adn_denoise_windows") + denoise_plan_text);
    if ((long)g.K * g.Wd >= (1L << 31)) return fail(ADN_ERR_INVALID, "adn_denoise_windows: windows x width must be < 2^31 frames");
    if (!aligned_to(spec, 8) || !aligned_to(out, 4)) return fail(ADN_ERR_INVALID, "adn_denoise_windows: spec must be 8-byte aligned, out 4-byte aligned");
    hipError_t e = adn::launch_denoise_windows(spec, n_clips, n_bins, g, out, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_denoise_windows: grid too large (n_clips x windows x 32x32 tiles >= 2^31)");
    ADN_HIP(e);
    return ADN_OK;
}

int adn_denoise_stitch(const float *y, int n_clips, int n_frames, int n_bins, int window, int overlap, int clamp, float *out, void *stream)
{
    if (!y || !out) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: null pointer");
    if (y == out) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: out may not alias y");
    if (n_clips < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: n_clips and n_bins must be >= 1");
    if (clamp != 0 && clamp != 1) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: clamp must be 0 or 1");
    adn::DenoiseGeom g;
    if (!adn::denoise_geom(n_frames, window, overlap, &g)) return fail(ADN_ERR_INVALID, std::string("adn_denoise_stitch") + denoise_plan_text);
    if ((long)g.K * g.Wd >= (1L << 31)) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: windows x width must be < 2^31 frames");
    const bool vec = ((g.T | g.Wd | g.S | g.V) & 3) == 0;          // the 16-byte path (launch_denoise_stitch takes it by the same rule)
    if (!aligned_to(y, vec ? 16 : 4) || !aligned_to(out, vec ? 16 : 4))
        return fail(ADN_ERR_INVALID, "adn_denoise_stitch: y and out must be 4-byte aligned (16-byte when n_frames, the window width, stride and overlap are all multiples of 4)");
    hipError_t e = adn::launch_denoise_stitch(y, n_clips, n_bins, g, clamp, out, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_denoise_stitch: grid too large (n_clips x n_bins x n_frames / 1024 >= 2^31)");
    ADN_HIP(e);
    return ADN_OK;
}

int adn_denoise_resynth(const float *y, const float *spec, int n_clips, long length, int n_fft, int hop, int window, int overlap,
                        float *audio_out, void *stream)
{
    if (!y || !spec || !audio_out) return fail(ADN_ERR_INVALID, "adn_denoise_resynth: null pointer");
    if (!gl_size_ok(n_fft)) return fail(ADN_ERR_INVALID, "adn_denoise_resynth: n_fft must be a power of two in [64, 4096]");
    if (hop < 1 || hop > n_fft / 4)
        return fail(ADN_ERR_INVALID, "adn_denoise_resynth: need 1 <= hop <= n_fft / 4 (at n_fft / 2 the window sum-of-squares of the tail samples falls to 2e-8)");
    if (n_clips < 1 || length < 1 || length >= (1L << 30)) return fail(ADN_ERR_INVALID, "adn_denoise_resynth: need n_clips >= 1 and 1 <= length < 2^30");
    adn::DenoiseGeom g;
    if (!adn::denoise_geom((int)(1 + length / hop), window, overlap, &g)) return fail(ADN_ERR_INVALID, std::string("adn_denoise_resynth") + denoise_plan_text);
    if ((long)g.K * g.Wd >= (1L << 31)) return fail(ADN_ERR_INVALID, "adn_denoise_resynth: windows x width must be < 2^31 frames");
    if (!aligned_to(spec, 8) || !aligned_to(y, 4) || !aligned_to(audio_out, 4))
        return fail(ADN_ERR_INVALID, "adn_denoise_resynth: spec must be 8-byte aligned, y and audio_out 4-byte aligned");
    hipError_t e = adn::launch_denoise_resynth(y, spec, n_clips, length, n_fft, hop, g, audio_out, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_denoise_resynth: grid too large (n_clips x length / 2048 >= 2^31)");
    ADN_LAUNCH(e, "adn_denoise_resynth");
    return ADN_OK;
}

/* ---- spectral baseline: noise tracking + Wiener gain (adn.h, "baseline") ----------------------------------------- */
// The parameters of a call (NULL = the defaults), refused outside their legal ranges, and the constants derived from them once.
static int spectral_consts(const char *who, const adn_spectral_params *params, adn::SpectralConsts *k)
{
    const std::string w(who);
    const adn_spectral_params defaults = {0.7f, 0.96f, 0.998f, 0.98f, 0.1f, 1.0f};
    const adn_spectral_params p = params ? *params : defaults;
    // written so that a NaN fails every test
    if (!(p.smooth >= 0.f && p.smooth < 1.f) || !(p.beta >= 0.f && p.beta < 1.f) || !(p.alpha >= 0.f && p.alpha < 1.f))
        return fail(ADN_ERR_INVALID, w + ": need 0 <= smooth, beta, alpha < 1");
    if (!(p.gamma > 0.f && p.gamma < 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 < gamma < 1");
    if (!(p.gain_floor > 0.f && p.gain_floor <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 < gain_floor <= 1");
    if (!(p.bias > 0.f && p.bias <= 100.f)) return fail(ADN_ERR_INVALID, w + ": need 0 < bias <= 100");
    k->smooth = p.smooth;
    k->one_minus_smooth = 1.f - p.smooth;
    k->beta = p.beta;
    k->gamma = p.gamma;
    k->growth = (1.f - p.gamma) / (1.f - p.beta);
    k->alpha = p.alpha;
    k->one_minus_alpha = 1.f - p.alpha;
    k->gain_floor = p.gain_floor;
    k->bias = p.bias;
    return ADN_OK;
}

int adn_spectral_gain(const float *spec, int n_clips, int n_frames, int n_bins, const adn_spectral_params *params,
                      const float *state_in, float *state_out, float *out, int width, int col0, void *stream)
{
    if (!spec || !out) return fail(ADN_ERR_INVALID, "adn_spectral_gain: null pointer");
    if (n_clips < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, "adn_spectral_gain: n_clips, n_frames and n_bins must be >= 1");
    if (col0 < 0 || width < 1 || (long)col0 + n_frames > width)
        return fail(ADN_ERR_INVALID, "adn_spectral_gain: need col0 >= 0 and col0 + n_frames <= width");
    adn::SpectralConsts k;
    const int rc = spectral_consts("adn_spectral_gain", params, &k);
    if (rc != ADN_OK) return rc;
    if (!aligned_to(spec, 8) || !aligned_to(out, 4) || !aligned_to(state_in, 4) || !aligned_to(state_out, 4))
        return fail(ADN_ERR_INVALID, "adn_spectral_gain: spec must be 8-byte aligned, out and the states 4-byte aligned");
    hipError_t e = adn::launch_spectral_gain(spec, n_clips, n_frames, n_bins, k, state_in, state_out, out, width, col0,
                                             static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_spectral_gain: grid too large (n_clips x ceil(n_bins / 64) >= 2^31)");
    ADN_LAUNCH(e, "adn_spectral_gain");
    return ADN_OK;
}

static_assert(ADN_SPECTRAL_MAX_ROWS == adn::SPECTRAL_MAX_ROWS && sizeof(adn_spectral_row) == sizeof(adn::SpectralRow),
              "adn.h and adn_internal.h disagree about the baseline's row table");

int adn_spectral_gain_windows(const float *windows, float *y, int n_rows, int n_steps, int n_bins, int window, int col0, int n_cols,
                              const adn_spectral_params *params, float *state, int n_slots, const adn_spectral_row *rows, void *stream)
{
    if (!windows || !y || !state) return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: null pointer");
    if (n_rows < 1 || n_steps < 1 || n_bins < 1 || window < 1 || n_cols < 1 || n_slots < 1)
        return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: n_rows, n_steps, n_bins, window, n_cols and n_slots must be >= 1");
    if (col0 < 0 || (long)col0 + n_cols > window)
        return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: need col0 >= 0 and col0 + n_cols <= window");
    if ((long)n_steps * n_cols >= (1L << 31))
        return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: n_steps x n_cols must be < 2^31 frames");
    adn::SpectralRows t = {};
    if (!rows) {
        if (n_rows > n_slots) return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: without rows, row i uses slot i: need n_rows <= n_slots");
    } else {
        if (n_rows > ADN_SPECTRAL_MAX_ROWS)
            return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: need n_rows <= ADN_SPECTRAL_MAX_ROWS with rows (call again for the rest)");
        int slots[ADN_SPECTRAL_MAX_ROWS];
        for (int i = 0; i < n_rows; ++i) {
            const adn_spectral_row r = rows[i];
            if (r.slot < 0 || r.slot >= n_slots) return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: a row's slot is outside [0, n_slots)");
            slots[i] = r.slot;
            t.row[i].slot = r.slot;
            t.row[i].fresh = r.fresh != 0;
        }
        std::sort(slots, slots + n_rows);                    // a tick pays for this check: n log n, not n^2
        if (std::adjacent_find(slots, slots + n_rows) != slots + n_rows)
            return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: a slot is named twice in one call");
        t.n = n_rows;
    }
    adn::SpectralConsts k;
    const int rc = spectral_consts("adn_spectral_gain_windows", params, &k);
    if (rc != ADN_OK) return rc;
    if (!aligned_to(windows, 4) || !aligned_to(y, 4) || !aligned_to(state, 4))
        return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: windows, y and state must be 4-byte aligned");
    hipError_t e = adn::launch_spectral_gain_windows(windows, y, n_rows, n_steps, n_bins, window, col0, n_cols, k, state, t,
                                                     static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue)
        return fail(ADN_ERR_INVALID, "adn_spectral_gain_windows: grid too large (n_rows x ceil(n_bins / 64) >= 2^31)");
    ADN_LAUNCH(e, "adn_spectral_gain_windows");
    return ADN_OK;
}

/* ---- dereverberation: WPE per bin, one channel or the channels of a recording jointly (adn.h, "dereverb", "dereverb multichannel") */
// The two entry points of a pair share one body: the single-channel one is the joint one at channels = 1, where the rules that need
// the channel count cannot fire.  What differs between them is passed in: the name in front of every message, what the messages
// call the batch dimension and one member of it, the sizing function they name, and the taps that params = NULL stands for -- 0: the
// operator's own (20), for the single-channel functions; 32 / channels for the joint ones, channels = 1 included.  Which kernel
// runs is the launcher's choice.
struct WpeCall {
    const char *name, *n_rows, *row, *sizer;
    int default_taps;
};
// (an illegal channel count is refused before the value is used)
static int joint_default_taps(int channels) { return 32 / (channels < 1 ? 1 : channels); }

// The parameters of a call (NULL = the defaults), refused outside their legal ranges; the message names the field.
static int wpe_consts(const char *who, const adn_wpe_params *params, int default_taps, adn::WpeConsts *k)
{
    const std::string w(who);
    adn_wpe_params defaults = {20, 3, 3, 1e-3f, 1e-3f};
    if (default_taps) defaults.taps = default_taps;
    const adn_wpe_params p = params ? *params : defaults;
    if (p.taps < 1 || p.taps > 32) return fail(ADN_ERR_INVALID, w + ": need 1 <= taps <= 32");
    if (p.delay < 1 || p.delay > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= delay <= 8");
    if (p.iterations < 1 || p.iterations > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= iterations <= 8");
    // written so that a NaN fails every test
    if (!(p.loading >= 1e-6f && p.loading <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 1e-6 <= loading <= 1");
    if (!(p.power_floor > 0.f && p.power_floor <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 < power_floor <= 1");
    k->K = p.taps;
    k->D = p.delay;
    k->I = p.iterations;
    k->loading = p.loading;
    k->rho = p.power_floor;
    return ADN_OK;
}

static int wpe_shape(const WpeCall &c, int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params,
                     adn::WpeConsts *k)
{
    const std::string w(c.name);
    if (n_groups < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, w + ": " + c.n_rows + ", n_frames and n_bins must be >= 1");
    if (channels < 1 || channels > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= channels <= 8");
    if ((long)n_groups * channels > 0x7fffffffL) return fail(ADN_ERR_INVALID, w + ": need n_groups * channels < 2^31");
    ADN_TRY(wpe_consts(c.name, params, c.default_taps, k));
    if (channels * k->K > 32) return fail(ADN_ERR_INVALID, w + ": need channels * taps <= 32");
    if (adn::wpe_grid(n_groups, channels, n_bins, k->K) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (" + c.n_rows + " x ceil(n_bins / bins per workgroup) >= 2^31)");
    return ADN_OK;
}

static int wpe_workspace_bytes(const WpeCall &c, int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params,
                               size_t *bytes)
{
    adn::WpeConsts k;
    if (!bytes) return fail(ADN_ERR_INVALID, std::string(c.name) + ": null pointer");
    ADN_TRY(wpe_shape(c, n_groups, channels, n_frames, n_bins, params, &k));
    *bytes = 0;                                          // R, P, the factor and the taps of a (group, bin) never leave the chip
    return ADN_OK;
}

static int wpe(const WpeCall &c, const float *spec, int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params,
               void *workspace, size_t workspace_bytes, float *spec_out, float *mag_out, int width, void *stream)
{
    const std::string w(c.name);
    adn::WpeConsts k;
    if (!spec || !spec_out) return fail(ADN_ERR_INVALID, w + ": null pointer (spec, spec_out)");
    ADN_TRY(wpe_shape(c, n_groups, channels, n_frames, n_bins, params, &k));
    if (mag_out && width < n_frames) return fail(ADN_ERR_INVALID, w + ": need width >= n_frames");
    if (!aligned_to(spec, 8) || !aligned_to(spec_out, 8) || !aligned_to(mag_out, 4))
        return fail(ADN_ERR_INVALID, w + ": spec and spec_out must be 8-byte aligned, mag_out 4-byte aligned");
    const size_t need = 0;                               // what c.sizer reports
    if (workspace_bytes < need || (need && !workspace)) return fail(ADN_ERR_WORKSPACE, w + ": workspace smaller than " + c.sizer);
    const char *a = reinterpret_cast<const char *>(spec), *b = reinterpret_cast<const char *>(spec_out);
    const size_t span = (size_t)n_groups * (size_t)channels * (size_t)n_frames * (size_t)n_bins * 2 * sizeof(float);
    if (a < b + span && b < a + span) return fail(ADN_ERR_INVALID, w + ": spec and spec_out may not overlap");
    ADN_LAUNCH(adn::launch_wpe(spec, n_groups, channels, n_frames, n_bins, k, spec_out, mag_out, width, static_cast<hipStream_t>(stream)),
               c.name);
    return ADN_OK;
}

int adn_wpe_workspace_bytes(int n_clips, int n_frames, int n_bins, const adn_wpe_params *params, size_t *bytes)
{
    return wpe_workspace_bytes({"adn_wpe_workspace_bytes", "n_clips", "clip", "", 0}, n_clips, 1, n_frames, n_bins, params, bytes);
}

int adn_wpe(const float *spec, int n_clips, int n_frames, int n_bins, const adn_wpe_params *params, void *workspace,
            size_t workspace_bytes, float *spec_out, float *mag_out, int width, void *stream)
{
    return wpe({"adn_wpe", "n_clips", "clip", "adn_wpe_workspace_bytes", 0}, spec, n_clips, 1, n_frames, n_bins, params, workspace,
               workspace_bytes, spec_out, mag_out, width, stream);
}

int adn_wpe_mc_workspace_bytes(int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params, size_t *bytes)
{
    return wpe_workspace_bytes({"adn_wpe_mc_workspace_bytes", "n_groups", "group", "", joint_default_taps(channels)}, n_groups, channels,
                               n_frames, n_bins, params, bytes);
}

int adn_wpe_mc(const float *spec, int n_groups, int channels, int n_frames, int n_bins, const adn_wpe_params *params, void *workspace,
               size_t workspace_bytes, float *spec_out, float *mag_out, int width, void *stream)
{
    return wpe({"adn_wpe_mc", "n_groups", "group", "adn_wpe_mc_workspace_bytes", joint_default_taps(channels)}, spec, n_groups, channels,
               n_frames, n_bins, params, workspace, workspace_bytes, spec_out, mag_out, width, stream);
}

/* ---- beamformer: mask-driven MVDR of the channels of a recording (adn.h, "beamform") ----------------------------- */
// The sizing function and the operator share one validation: `who` is the name in front of every message.
// The rules adn_mvdr and the streaming form share: the channel count and the three fields both parameter structs have.
static int mvdr_fields(const std::string &w, int channels, int ref_channel, float loading, float mask_floor, adn::MvdrConsts *k)
{
    if (ref_channel < 0 || ref_channel >= channels) return fail(ADN_ERR_INVALID, w + ": need 0 <= ref_channel < channels");
    // written so that a NaN fails every test
    if (!(loading >= 1e-6f && loading <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 1e-6 <= loading <= 1");
    if (!(mask_floor >= 1e-6f && mask_floor <= 0.25f)) return fail(ADN_ERR_INVALID, w + ": need 1e-6 <= mask_floor <= 0.25");
    k->ref = ref_channel;
    k->loading = loading;
    k->rho = mask_floor;
    k->one_minus_rho = 1.f - mask_floor;
    return ADN_OK;
}

static int mvdr_shape(const char *who, int n_groups, int channels, int n_frames, int n_bins, const adn_mvdr_params *params,
                      adn::MvdrConsts *k)
{
    const std::string w(who);
    if (n_groups < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, w + ": n_groups, n_frames and n_bins must be >= 1");
    if (channels < 1 || channels > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= channels <= 8");
    if ((long)n_groups * channels > 0x7fffffffL) return fail(ADN_ERR_INVALID, w + ": need n_groups * channels < 2^31");
    const adn_mvdr_params defaults = {0, 1e-3f, 1e-3f};
    const adn_mvdr_params p = params ? *params : defaults;
    ADN_TRY(mvdr_fields(w, channels, p.ref_channel, p.loading, p.mask_floor, k));
    if (adn::mvdr_grid(n_groups, channels, n_bins) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (n_groups x ceil(n_bins / bins per workgroup) >= 2^31)");
    return ADN_OK;
}

int adn_mvdr_workspace_bytes(int n_groups, int channels, int n_frames, int n_bins, const adn_mvdr_params *params, size_t *bytes)
{
    adn::MvdrConsts k;
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_mvdr_workspace_bytes: null pointer");
    ADN_TRY(mvdr_shape("adn_mvdr_workspace_bytes", n_groups, channels, n_frames, n_bins, params, &k));
    *bytes = 0;                                          // the covariances, the factor and the filter of a (group, bin) never leave the chip
    return ADN_OK;
}

int adn_mvdr(const float *spec, const float *mag, int mag_width, int n_groups, int channels, int n_frames, int n_bins,
             const adn_mvdr_params *params, void *workspace, size_t workspace_bytes, float *spec_out, float *mag_out, int width,
             void *stream)
{
    const std::string w("adn_mvdr");
    adn::MvdrConsts k;
    if (!spec || !mag || !spec_out) return fail(ADN_ERR_INVALID, w + ": null pointer (spec, mag, spec_out)");
    ADN_TRY(mvdr_shape("adn_mvdr", n_groups, channels, n_frames, n_bins, params, &k));
    if (mag_width < n_frames) return fail(ADN_ERR_INVALID, w + ": need mag_width >= n_frames");
    if (mag_out && width < n_frames) return fail(ADN_ERR_INVALID, w + ": need width >= n_frames");
    if (!aligned_to(spec, 8) || !aligned_to(spec_out, 8) || !aligned_to(mag, 4) || !aligned_to(mag_out, 4))
        return fail(ADN_ERR_INVALID, w + ": spec and spec_out must be 8-byte aligned, mag and mag_out 4-byte aligned");
    const size_t need = 0;                               // what adn_mvdr_workspace_bytes reports
    if (workspace_bytes < need || (need && !workspace))
        return fail(ADN_ERR_WORKSPACE, w + ": workspace smaller than adn_mvdr_workspace_bytes");
    const size_t cells = (size_t)n_groups * (size_t)n_bins;
    const auto overlap = [](const void *p, size_t np, const void *q, size_t nq) {
        const char *a = reinterpret_cast<const char *>(p), *b = reinterpret_cast<const char *>(q);
        return a < b + nq && b < a + np;
    };
    const size_t in_spec = cells * channels * n_frames * 2 * sizeof(float), out_spec = cells * n_frames * 2 * sizeof(float);
    const size_t in_mag = cells * channels * mag_width * sizeof(float), out_mag = mag_out ? cells * width * sizeof(float) : 0;
    if (overlap(spec, in_spec, spec_out, out_spec) || overlap(mag, in_mag, spec_out, out_spec))
        return fail(ADN_ERR_INVALID, w + ": spec_out may not overlap spec or mag");
    if (mag_out && (overlap(spec, in_spec, mag_out, out_mag) || overlap(mag, in_mag, mag_out, out_mag) ||
                    overlap(spec_out, out_spec, mag_out, out_mag)))
        return fail(ADN_ERR_INVALID, w + ": mag_out may not overlap spec, mag or spec_out");
    ADN_LAUNCH(adn::launch_mvdr(spec, mag, mag_width, n_groups, channels, n_frames, n_bins, k, spec_out, mag_out, width,
                                static_cast<hipStream_t>(stream)),
               "adn_mvdr");
    return ADN_OK;
}

/* ---- streaming denoiser: plan, state, analysis, emit (adn.h, "stream") ------------------------------------------- */
static const char *stream_plan_text = ": need a power-of-two n_fft in [64, 4096], 1 <= hop <= n_fft / 4, window >= 16, block >= 1, "
                                      "lookahead >= 0, block + lookahead <= window, n_streams >= 1 and 1 <= max_steps <= 65536";

// The limits of a call of n_steps steps from `first`, then what it covers (adn_internal.h, stream_call_of).
// (not static: csrc/echo/echo_api.hip, the C ABI of libadn_echo.so, puts the same two checks in front of adn_aec_stream; adn_host.h)
int stream_call(const char *who, const adn::StreamGeom &g, long first, int n_steps, long final_length, adn::StreamCall *c)
{
    const std::string w(who);
    if (first < 0 || n_steps < 1) return fail(ADN_ERR_INVALID, w + ": need first_step >= 0 and n_steps >= 1");
    if (n_steps > g.S - 1) return fail(ADN_ERR_INVALID, w + ": n_steps exceeds the max_steps the state was sized for");
    if (final_length < -1 || final_length == 0 || final_length >= (1L << 30))
        return fail(ADN_ERR_INVALID, w + ": final_length must be -1 (the stream runs) or the stream's length, 1 <= length < 2^30");
    const long B = g.B, D = g.B + g.A, hop = g.hop;
    if (first >= (1L << 30)) return fail(ADN_ERR_INVALID, w + ": step index too large");
    const long last = first + n_steps - 1;
    // sample positions are 32-bit inside the kernels: the last position a call touches stays below 2^30 (flush before that)
    if ((last * B + D) * hop + 2L * g.n_fft >= (1L << 30))
        return fail(ADN_ERR_INVALID, w + ": the steps reach past sample 2^30 of the stream (32-bit positions inside the kernels); flush the stream before");
    if (final_length > 0) {
        const long T = 1 + final_length / hop, K = (T + B - 1) / B;
        if (last >= K) return fail(ADN_ERR_INVALID, w + ": steps past the last step ceil((1 + final_length / hop) / block) of the stream");
    }
    *c = adn::stream_call_of(g, first, n_steps, final_length);
    return ADN_OK;
}

int adn_stream_plan(int n_fft, int hop, int window, int block, int lookahead, long received, long *steps_done, long *emitted,
                    long *latency)
{
    adn::StreamGeom g;
    if (!adn::stream_geom(1, n_fft, hop, window, block, lookahead, 1, &g)) return fail(ADN_ERR_INVALID, std::string("adn_stream_plan") + stream_plan_text);
    if (received < 0 || received >= (1L << 40)) return fail(ADN_ERR_INVALID, "adn_stream_plan: need 0 <= received < 2^40");
    const long r = received - n_fft / 2 - (long)(block + lookahead - 1) * hop;
    const long steps = r < 0 ? 0 : r / ((long)block * hop) + 1;
    const long out = steps * block * hop - n_fft / 2;
    if (steps_done) *steps_done = steps;
    if (emitted) *emitted = out > 0 ? out : 0;
    if (latency) *latency = (long)(block + lookahead - 1) * hop + n_fft;
    return ADN_OK;
}

int adn_stream_state_bytes(int n_streams, int n_fft, int hop, int window, int block, int lookahead, int max_steps, size_t *bytes)
{
    adn::StreamGeom g;
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_stream_state_bytes: null pointer");
    if (!adn::stream_geom(n_streams, n_fft, hop, window, block, lookahead, max_steps, &g))
        return fail(ADN_ERR_INVALID, std::string("adn_stream_state_bytes") + stream_plan_text);
    *bytes = (size_t)g.total * sizeof(float);
    return ADN_OK;
}

int stream_state(const char *who, void *state, size_t state_bytes, int n_streams, int n_fft, int hop, int window, int block,
                        int lookahead, int max_steps, adn::StreamGeom *g)
{
    const std::string w(who);
    if (!state) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!adn::stream_geom(n_streams, n_fft, hop, window, block, lookahead, max_steps, g)) return fail(ADN_ERR_INVALID, w + stream_plan_text);
    if (state_bytes < (size_t)g->total * sizeof(float)) return fail(ADN_ERR_WORKSPACE, w + ": state smaller than adn_stream_state_bytes");
    if (!aligned_to(state, 8)) return fail(ADN_ERR_INVALID, w + ": state must be 8-byte aligned");
    return ADN_OK;
}

int adn_stream_reset(void *state, size_t state_bytes, int n_streams, int n_fft, int hop, int window, int block, int lookahead,
                     int max_steps, void *stream)
{
    adn::StreamGeom g;
    const int rc = stream_state("adn_stream_reset", state, state_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, &g);
    if (rc != ADN_OK) return rc;
    ADN_HIP(hipMemsetAsync(state, 0, (size_t)g.total * sizeof(float), static_cast<hipStream_t>(stream)));
    return ADN_OK;
}

int adn_stream_analyze(void *state, size_t state_bytes, const float *audio, long audio_stride, int n_streams, long first_step,
                       int n_steps, long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                       float *windows_out, void *stream)
{
    adn::StreamGeom g;
    adn::StreamCall c;
    int rc = stream_state("adn_stream_analyze", state, state_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, &g);
    if (rc != ADN_OK) return rc;
    if (!audio || !windows_out) return fail(ADN_ERR_INVALID, "adn_stream_analyze: null pointer");
    if (!aligned_to(audio, 4) || !aligned_to(windows_out, 4)) return fail(ADN_ERR_INVALID, "adn_stream_analyze: audio and windows_out must be 4-byte aligned");
    rc = stream_call("adn_stream_analyze", g, first_step, n_steps, final_length, &c);
    if (rc != ADN_OK) return rc;
    const long n_new = (c.L >= 0 && c.L < c.end ? c.L : c.end) - (long)c.base;
    if (audio_stride < 0 || (n_streams > 1 && audio_stride < n_new))
        return fail(ADN_ERR_INVALID, "adn_stream_analyze: audio_stride is smaller than the samples the steps bring");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = adn::launch_stream_frames(audio, audio_stride, n_streams, g, c, static_cast<float *>(state), st);
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stream_analyze: grid too large");
    ADN_LAUNCH(e, "adn_stream_analyze");
    e = adn::launch_stream_windows(static_cast<const float *>(state), n_streams, g, c, windows_out, st);
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stream_analyze: grid too large (n_streams x n_steps x 32x32 tiles >= 2^31)");
    ADN_HIP(e);
    return ADN_OK;
}

int adn_stream_emit(void *state, size_t state_bytes, const float *y, int n_streams, long first_step, int n_steps, long final_length,
                    int n_fft, int hop, int window, int block, int lookahead, int max_steps, float *audio_out, long out_stride,
                    void *stream)
{
    adn::StreamGeom g;
    adn::StreamCall c;
    int rc = stream_state("adn_stream_emit", state, state_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, &g);
    if (rc != ADN_OK) return rc;
    if (!y) return fail(ADN_ERR_INVALID, "adn_stream_emit: null pointer");
    rc = stream_call("adn_stream_emit", g, first_step, n_steps, final_length, &c);
    if (rc != ADN_OK) return rc;
    const long n_out = c.p_out > c.p_first ? (long)c.p_out - c.p_first : 0;
    if (n_out > 0 && !audio_out) return fail(ADN_ERR_INVALID, "adn_stream_emit: null pointer");
    if (out_stride < 0 || (n_streams > 1 && out_stride < n_out))
        return fail(ADN_ERR_INVALID, "adn_stream_emit: out_stride is smaller than the samples the steps emit");
    if (!aligned_to(y, 4) || !aligned_to(audio_out, 4)) return fail(ADN_ERR_INVALID, "adn_stream_emit: y and audio_out must be 4-byte aligned");
    hipError_t e = adn::launch_stream_emit(y, n_streams, g, c, static_cast<float *>(state), audio_out, out_stride,
                                           static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_stream_emit: grid too large");
    ADN_LAUNCH(e, "adn_stream_emit");
    return ADN_OK;
}

/* ---- stream pool: independent streams in one state, their ready steps batched (adn.h, "stream pool") ---------------- */
static_assert(ADN_STREAM_POOL_MAX_ROWS == adn::STREAM_POOL_MAX_ROWS && sizeof(adn_stream_pool_row) == sizeof(adn::StreamPoolRow),
              "adn.h and adn_internal.h disagree about the pool's row table");
static const char *stream_pool_text = ": need the plan of the stream section (power-of-two n_fft in [64, 4096], 1 <= hop <= n_fft / 4, "
                                      "window >= 16, block >= 1, lookahead >= 0, block + lookahead <= window), 1 <= n_slots <= 2^20 and "
                                      "n_fft - hop + (block + lookahead - 1) hop + n_fft / 2 + block hop <= ring_samples <= 2^28";

// (pool_state, pool_rows and pool_recordings are not static: csrc/call/call_api.hip, the C ABI of libadn_call.so, puts the same
// checks in front of its pool operators; PoolState and their declarations are adn_host.h's)
int pool_state(const char *who, void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
                      int lookahead, long ring, PoolState *p)
{
    const std::string w(who);
    if (!state) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!adn::stream_pool_geom(n_slots, n_fft, hop, window, block, lookahead, ring, &p->g, &p->ring_off, &p->total))
        return fail(ADN_ERR_INVALID, w + stream_pool_text);
    if (state_bytes < (size_t)p->total * sizeof(float)) return fail(ADN_ERR_WORKSPACE, w + ": state smaller than adn_stream_pool_state_bytes");
    if (!aligned_to(state, 8)) return fail(ADN_ERR_INVALID, w + ": state must be 8-byte aligned");
    p->R = ring;
    return ADN_OK;
}

// The row table of a call, every row inside the stream section's limits; max_new / max_span: the most frames a row transforms and
// the most positions a row's emit covers (the grids are sized for them); max_out: the most samples a row writes out.
int pool_rows(const char *who, const PoolState &p, int n_slots, const adn_stream_pool_row *rows, int n_rows,
              adn::StreamPoolRows *t, int *max_new, int *max_span, long *max_out)
{
    const std::string w(who);
    if (!rows) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_rows < 1 || n_rows > ADN_STREAM_POOL_MAX_ROWS)
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_rows <= ADN_STREAM_POOL_MAX_ROWS (call again for the rest)");
    *max_new = *max_span = 0;
    *max_out = 0;
    for (int i = 0; i < n_rows; ++i) {
        const adn_stream_pool_row r = rows[i];
        if (r.slot < 0 || r.slot >= n_slots) return fail(ADN_ERR_INVALID, w + ": a row's slot is outside [0, n_slots)");
        for (int j = 0; j < i; ++j)
            if (rows[j].slot == r.slot) return fail(ADN_ERR_INVALID, w + ": a slot is named twice in one call (one step per stream and call)");
        adn::StreamCall c;
        const int rc = stream_call(who, p.g, r.step, 1, r.final_length, &c);
        if (rc != ADN_OK) return rc;
        if (c.f_new1 - c.f_new0 > *max_new) *max_new = c.f_new1 - c.f_new0;
        if (c.p_end - c.p_begin > *max_span) *max_span = c.p_end - c.p_begin;
        if ((long)c.p_out - c.p_first > *max_out) *max_out = (long)c.p_out - c.p_first;
        t->row[i].slot = r.slot;
        t->row[i].step = r.step;
        t->row[i].final_length = r.final_length;
    }
    t->ring_off = p.ring_off;
    t->R = (int)p.R;
    t->n = n_rows;
    return ADN_OK;
}

// The rows of a call on RECORDINGS of `channels` streams (adn.h, adn_wpe_mc_stream_pool), pool_rows passed: recording r owns
// the slots r C ... r C + C - 1, a group is C consecutive rows that name them in channel order and agree in step and final_length.
int pool_recordings(const char *who, int n_slots, int channels, const adn_stream_pool_row *rows, int n_rows)
{
    const std::string w(who);
    if (n_slots % channels) return fail(ADN_ERR_INVALID, w + ": n_slots must be a multiple of channels");
    if (n_rows % channels) return fail(ADN_ERR_INVALID, w + ": n_rows must be a multiple of channels (a recording is channels consecutive rows)");
    for (int i = 0; i < n_rows; i += channels) {
        if (rows[i].slot % channels)
            return fail(ADN_ERR_INVALID, w + ": a group's first slot must be a multiple of channels (recording r owns slots r channels ...)");
        for (int c = 1; c < channels; ++c) {
            if (rows[i + c].slot != rows[i].slot + c)
                return fail(ADN_ERR_INVALID, w + ": a group's slots must be consecutive, in channel order");
            if (rows[i + c].step != rows[i].step || rows[i + c].final_length != rows[i].final_length)
                return fail(ADN_ERR_INVALID, w + ": the rows of a group must agree in step and final_length");
        }
    }
    return ADN_OK;
}

int adn_stream_pool_state_bytes(int n_slots, int n_fft, int hop, int window, int block, int lookahead, long ring_samples, size_t *bytes)
{
    PoolState p;
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_stream_pool_state_bytes: null pointer");
    if (!adn::stream_pool_geom(n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p.g, &p.ring_off, &p.total))
        return fail(ADN_ERR_INVALID, std::string("adn_stream_pool_state_bytes") + stream_pool_text);
    *bytes = (size_t)p.total * sizeof(float);
    return ADN_OK;
}

int adn_stream_pool_reset(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block, int lookahead,
                          long ring_samples, int slot, void *stream)
{
    PoolState p;
    const int rc = pool_state("adn_stream_pool_reset", state, state_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p);
    if (rc != ADN_OK) return rc;
    if (slot < -1 || slot >= n_slots) return fail(ADN_ERR_INVALID, "adn_stream_pool_reset: slot must be -1 (all) or in [0, n_slots)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *s = static_cast<float *>(state);
    if (slot < 0) {
        ADN_HIP(hipMemsetAsync(s, 0, (size_t)p.total * sizeof(float), st));
        return ADN_OK;
    }
    const long F = n_fft / 2 + 1, keep = n_fft - hop;
    const long off[4] = {p.g.x_off + slot * 2 * F * p.g.RX, p.g.mag_off + slot * F * p.g.RM, p.g.tail_off + slot * keep * p.g.S,
                         p.ring_off + slot * p.R};
    const long len[4] = {2 * F * p.g.RX, F * p.g.RM, keep * p.g.S, p.R};
    for (int i = 0; i < 4; ++i) ADN_HIP(hipMemsetAsync(s + off[i], 0, (size_t)len[i] * sizeof(float), st));
    return ADN_OK;
}

int adn_stream_pool_write(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block, int lookahead,
                          long ring_samples, int slot, const float *audio, long n, long position, void *stream)
{
    PoolState p;
    const int rc = pool_state("adn_stream_pool_write", state, state_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p);
    if (rc != ADN_OK) return rc;
    if (slot < 0 || slot >= n_slots) return fail(ADN_ERR_INVALID, "adn_stream_pool_write: slot is outside [0, n_slots)");
    if (n < 0 || n > p.R) return fail(ADN_ERR_INVALID, "adn_stream_pool_write: need 0 <= n <= ring_samples");
    if (position < 0 || position + n >= (1L << 30))
        return fail(ADN_ERR_INVALID, "adn_stream_pool_write: need position >= 0 and position + n < 2^30 (32-bit positions inside the kernels)");
    if (n == 0) return ADN_OK;
    if (!audio) return fail(ADN_ERR_INVALID, "adn_stream_pool_write: null pointer");
    if (!aligned_to(audio, 4)) return fail(ADN_ERR_INVALID, "adn_stream_pool_write: audio must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ring = static_cast<float *>(state) + p.ring_off + slot * p.R;
    const long at = position % p.R, head = n < p.R - at ? n : p.R - at;
    ADN_HIP(hipMemcpyAsync(ring + at, audio, (size_t)head * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (n > head) ADN_HIP(hipMemcpyAsync(ring, audio + head, (size_t)(n - head) * sizeof(float), hipMemcpyDeviceToDevice, st));
    return ADN_OK;
}

int adn_stream_pool_analyze(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block, int lookahead,
                            long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *windows_out, void *stream)
{
    PoolState p;
    adn::StreamPoolRows t = {};
    int max_new, max_span;
    long max_out;
    int rc = pool_state("adn_stream_pool_analyze", state, state_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p);
    if (rc != ADN_OK) return rc;
    if (!windows_out) return fail(ADN_ERR_INVALID, "adn_stream_pool_analyze: null pointer");
    if (!aligned_to(windows_out, 4)) return fail(ADN_ERR_INVALID, "adn_stream_pool_analyze: windows_out must be 4-byte aligned");
    rc = pool_rows("adn_stream_pool_analyze", p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out);
    if (rc != ADN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ADN_LAUNCH(adn::launch_stream_pool_frames(p.g, t, max_new, static_cast<float *>(state), st), "adn_stream_pool_analyze");
    ADN_HIP(adn::launch_stream_pool_windows(static_cast<const float *>(state), p.g, t, windows_out, st));
    return ADN_OK;
}

int adn_stream_pool_emit(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block, int lookahead,
                         long ring_samples, const adn_stream_pool_row *rows, int n_rows, const float *y, float *audio_out,
                         long out_stride, void *stream)
{
    PoolState p;
    adn::StreamPoolRows t = {};
    int max_new, max_span;
    long max_out;
    int rc = pool_state("adn_stream_pool_emit", state, state_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p);
    if (rc != ADN_OK) return rc;
    if (!y) return fail(ADN_ERR_INVALID, "adn_stream_pool_emit: null pointer");
    rc = pool_rows("adn_stream_pool_emit", p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out);
    if (rc != ADN_OK) return rc;
    if (max_out > 0 && !audio_out) return fail(ADN_ERR_INVALID, "adn_stream_pool_emit: null pointer");
    if (out_stride < (long)block * hop + n_fft / 2)
        return fail(ADN_ERR_INVALID, "adn_stream_pool_emit: out_stride must be at least block hop + n_fft / 2, the most a step emits");
    if (!aligned_to(y, 4) || !aligned_to(audio_out, 4)) return fail(ADN_ERR_INVALID, "adn_stream_pool_emit: y and audio_out must be 4-byte aligned");
    ADN_LAUNCH(adn::launch_stream_pool_emit(y, p.g, t, max_span, static_cast<float *>(state), audio_out, out_stride,
                                            static_cast<hipStream_t>(stream)), "adn_stream_pool_emit");
    return ADN_OK;
}

/* ---- streaming dereverberation: recursive WPE, one channel or jointly (adn.h, "dereverb stream", "dereverb stream multichannel") */
// One body per pair, as for the offline operator above (WpeCall).  The parameters of a call on `channels` channels (NULL = the
// defaults), refused outside their legal ranges, then the rules that need the channel count.  k->K is the taps PER CHANNEL.
static int wpe_stream_consts(const char *who, int channels, const adn_wpe_stream_params *params, int default_taps,
                             adn::WpeStreamConsts *k)
{
    const std::string w(who);
    if (channels < 1 || channels > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= channels <= 8");
    adn_wpe_stream_params defaults = {20, 3, 0.99f, 300.f, 0.01f, 0.9f};
    if (default_taps) defaults.taps = default_taps;
    const adn_wpe_stream_params p = params ? *params : defaults;
    if (p.taps < 1 || p.taps > 32) return fail(ADN_ERR_INVALID, w + ": need 1 <= taps <= 32");
    if (p.delay < 1 || p.delay > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= delay <= 8");
    // written so that a NaN fails every test
    if (!(p.forget >= 0.95f && p.forget <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0.95 <= forget <= 1");
    if (!(p.loading >= 1.f && p.loading <= 1e6f)) return fail(ADN_ERR_INVALID, w + ": need 1 <= loading <= 1e6");
    if (!(p.power_floor > 0.f && p.power_floor <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 < power_floor <= 1");
    if (!(p.smooth >= 0.f && p.smooth < 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 <= smooth < 1");
    k->K = p.taps;
    k->D = p.delay;
    k->alpha = p.forget;
    k->p0 = 1.f / p.loading;
    k->rho = p.power_floor;
    k->beta = p.smooth;
    k->one_minus_beta = 1.f - p.smooth;
    if (channels * p.taps > 32) return fail(ADN_ERR_INVALID, w + ": need channels * taps <= 32");
    // the window 1 / (1 - forget) must hold twice the N unknowns (adn.h); in double, on the fp32 value the kernel uses
    if (channels >= 2 && !(2.0 * (double)(channels * p.taps) * (1.0 - (double)p.forget) <= 1.0))
        return fail(ADN_ERR_INVALID, w + ": need 2 channels taps (1 - forget) <= 1 with more than one channel (forget too low for the stacked size)");
    return ADN_OK;
}

static size_t wpe_stream_bytes(int n_slots, int n_bins, int channels, const adn::WpeStreamConsts &k)
{
    return (size_t)n_slots * (size_t)n_bins * (size_t)adn::wpe_stream_record_floats(channels, k.K, k.D) * sizeof(float);
}

// The WPE state of a call: n_slots x n_bins records, 8-byte aligned, at least what c.sizer reports.
static int wpe_stream_state(const WpeCall &c, const void *wstate, size_t wstate_bytes, int n_slots, int n_bins, int channels,
                            const adn::WpeStreamConsts &k)
{
    const std::string w(c.name);
    if (!wstate) return fail(ADN_ERR_INVALID, w + ": null pointer (the WPE state)");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    if (wstate_bytes < wpe_stream_bytes(n_slots, n_bins, channels, k))
        return fail(ADN_ERR_WORKSPACE, w + ": the WPE state is smaller than " + c.sizer);
    if (!aligned_to(wstate, 8)) return fail(ADN_ERR_INVALID, w + ": the WPE state must be 8-byte aligned");
    return ADN_OK;
}

static int wpe_stream_state_bytes(const WpeCall &c, int n_slots, int channels, int n_bins, const adn_wpe_stream_params *params,
                                  size_t *bytes)
{
    const std::string w(c.name);
    adn::WpeStreamConsts k;
    if (!bytes) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    ADN_TRY(wpe_stream_consts(c.name, channels, params, c.default_taps, &k));
    *bytes = wpe_stream_bytes(n_slots, n_bins, channels, k);
    return ADN_OK;
}

static int wpe_online(const WpeCall &c, const float *spec, int n_groups, int channels, int n_frames, int n_bins, long first_frame,
                      const adn_wpe_stream_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out,
                      float *mag_out, int width, int col0, void *stream)
{
    const std::string w(c.name);
    adn::WpeStreamConsts k;
    if (!spec || !spec_out) return fail(ADN_ERR_INVALID, w + ": null pointer (spec, spec_out)");
    if (n_groups < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, w + ": " + c.n_rows + ", n_frames and n_bins must be >= 1");
    if (first_frame < 0 || first_frame + n_frames >= (1L << 31))
        return fail(ADN_ERR_INVALID, w + ": need first_frame >= 0 and first_frame + n_frames < 2^31");
    ADN_TRY(wpe_stream_consts(c.name, channels, params, c.default_taps, &k));
    if ((long)n_groups * channels > 0x7fffffffL) return fail(ADN_ERR_INVALID, w + ": need n_groups * channels < 2^31");
    ADN_TRY(wpe_stream_state(c, state, state_bytes, n_slots, n_bins, channels, k));
    if (n_groups > n_slots) return fail(ADN_ERR_INVALID, w + ": " + c.row + " i uses slot i: need " + c.n_rows + " <= n_slots");
    if (mag_out && (col0 < 0 || width < 1 || (long)col0 + n_frames > width))
        return fail(ADN_ERR_INVALID, w + ": need col0 >= 0 and col0 + n_frames <= width");
    if (!aligned_to(spec, 8) || !aligned_to(spec_out, 8) || !aligned_to(mag_out, 4))
        return fail(ADN_ERR_INVALID, w + ": spec and spec_out must be 8-byte aligned, mag_out 4-byte aligned");
    const char *a = reinterpret_cast<const char *>(spec), *b = reinterpret_cast<const char *>(spec_out);
    const size_t span = (size_t)n_groups * (size_t)channels * (size_t)n_frames * (size_t)n_bins * 2 * sizeof(float);
    if (a < b + span && b < a + span) return fail(ADN_ERR_INVALID, w + ": spec and spec_out may not overlap");
    if (adn::wpe_stream_grid(n_groups, n_bins) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (" + c.n_rows + " x ceil(n_bins / 8) >= 2^31)");
    ADN_LAUNCH(adn::launch_wpe_online(spec, n_groups, channels, n_frames, n_bins, (int)first_frame, k, static_cast<float *>(state),
                                      spec_out, mag_out, width, col0, static_cast<hipStream_t>(stream)), c.name);
    return ADN_OK;
}

static int wpe_stream(const WpeCall &c, void *sstate, size_t sstate_bytes, float *y, int n_streams, int channels, long first_step,
                      int n_steps, long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                      const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream)
{
    const std::string w(c.name);
    adn::StreamGeom g;
    adn::StreamCall call;
    adn::WpeStreamConsts k;
    ADN_TRY(stream_state(c.name, sstate, sstate_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, &g));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    ADN_TRY(stream_call(c.name, g, first_step, n_steps, final_length, &call));
    ADN_TRY(wpe_stream_consts(c.name, channels, params, c.default_taps, &k));
    if (n_streams % channels) return fail(ADN_ERR_INVALID, w + ": n_streams must be a multiple of channels");
    ADN_TRY(wpe_stream_state(c, wpe_state, wpe_state_bytes, n_streams / channels, n_fft / 2 + 1, channels, k));
    ADN_LAUNCH(adn::launch_wpe_stream(static_cast<float *>(sstate), y, n_streams, channels, g, call, k, static_cast<float *>(wpe_state),
                                      static_cast<hipStream_t>(stream)), c.name);
    return ADN_OK;
}

int adn_wpe_stream_state_bytes(int n_slots, int n_bins, const adn_wpe_stream_params *params, size_t *bytes)
{
    return wpe_stream_state_bytes({"adn_wpe_stream_state_bytes", "n_rows", "row", "", 0}, n_slots, 1, n_bins, params, bytes);
}

int adn_wpe_online(const float *spec, int n_rows, int n_frames, int n_bins, long first_frame, const adn_wpe_stream_params *params,
                   void *state, size_t state_bytes, int n_slots, float *spec_out, float *mag_out, int width, int col0, void *stream)
{
    return wpe_online({"adn_wpe_online", "n_rows", "row", "adn_wpe_stream_state_bytes", 0}, spec, n_rows, 1, n_frames, n_bins,
                      first_frame, params, state, state_bytes, n_slots, spec_out, mag_out, width, col0, stream);
}

int adn_wpe_stream(void *sstate, size_t sstate_bytes, float *y, int n_streams, long first_step, int n_steps,
                   long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                   const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream)
{
    return wpe_stream({"adn_wpe_stream", "n_rows", "row", "adn_wpe_stream_state_bytes", 0}, sstate, sstate_bytes, y, n_streams, 1,
                      first_step, n_steps, final_length, n_fft, hop, window, block, lookahead, max_steps, params, wpe_state,
                      wpe_state_bytes, stream);
}

int adn_wpe_mc_stream_state_bytes(int n_slots, int channels, int n_bins, const adn_wpe_stream_params *params, size_t *bytes)
{
    return wpe_stream_state_bytes({"adn_wpe_mc_stream_state_bytes", "n_groups", "group", "", joint_default_taps(channels)}, n_slots,
                                  channels, n_bins, params, bytes);
}

int adn_wpe_mc_online(const float *spec, int n_groups, int channels, int n_frames, int n_bins, long first_frame,
                      const adn_wpe_stream_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out, float *mag_out,
                      int width, int col0, void *stream)
{
    return wpe_online({"adn_wpe_mc_online", "n_groups", "group", "adn_wpe_mc_stream_state_bytes", joint_default_taps(channels)}, spec,
                      n_groups, channels, n_frames, n_bins, first_frame, params, state, state_bytes, n_slots, spec_out, mag_out, width,
                      col0, stream);
}

int adn_wpe_mc_stream(void *sstate, size_t sstate_bytes, float *y, int n_streams, int channels, long first_step, int n_steps,
                      long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                      const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream)
{
    return wpe_stream({"adn_wpe_mc_stream", "n_groups", "group", "adn_wpe_mc_stream_state_bytes", joint_default_taps(channels)}, sstate,
                      sstate_bytes, y, n_streams, channels, first_step, n_steps, final_length, n_fft, hop, window, block, lookahead,
                      max_steps, params, wpe_state, wpe_state_bytes, stream);
}

// The pool's rows are single-channel streams: it shares the parameter and the state checks (channels = 1) and keeps its own rows.
int adn_wpe_stream_pool(void *pstate, size_t pstate_bytes, int n_slots, int n_fft, int hop, int window, int block,
                        int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                        const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream)
{
    const WpeCall c = {"adn_wpe_stream_pool", "n_rows", "row", "adn_wpe_stream_state_bytes", 0};
    PoolState p;
    adn::StreamPoolRows t = {};
    adn::WpeStreamConsts k;
    int max_new, max_span;
    long max_out;
    ADN_TRY(pool_state(c.name, pstate, pstate_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, "adn_wpe_stream_pool: the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, "adn_wpe_stream_pool: null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, "adn_wpe_stream_pool: y must be 4-byte aligned");
    ADN_TRY(pool_rows(c.name, p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out));
    ADN_TRY(wpe_stream_consts(c.name, 1, params, c.default_taps, &k));
    ADN_TRY(wpe_stream_state(c, wpe_state, wpe_state_bytes, n_slots, n_fft / 2 + 1, 1, k));
    ADN_LAUNCH(adn::launch_wpe_stream_pool(static_cast<float *>(pstate), y, p.g, t, k, static_cast<float *>(wpe_state),
                                           static_cast<hipStream_t>(stream)), c.name);
    return ADN_OK;
}

// The pool's rows are the channels of recordings: the checks of the pool call, of the joint parameters and of the groups.
int adn_wpe_mc_stream_pool(void *pstate, size_t pstate_bytes, int n_slots, int channels, int n_fft, int hop, int window, int block,
                           int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                           const adn_wpe_stream_params *params, void *wpe_state, size_t wpe_state_bytes, void *stream)
{
    const WpeCall c = {"adn_wpe_mc_stream_pool", "n_groups", "group", "adn_wpe_mc_stream_state_bytes", joint_default_taps(channels)};
    const std::string w(c.name);
    PoolState p;
    adn::StreamPoolRows t = {};
    adn::WpeStreamConsts k;
    int max_new, max_span;
    long max_out;
    ADN_TRY(pool_state(c.name, pstate, pstate_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    ADN_TRY(pool_rows(c.name, p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out));
    ADN_TRY(wpe_stream_consts(c.name, channels, params, c.default_taps, &k));
    ADN_TRY(pool_recordings(c.name, n_slots, channels, rows, n_rows));
    ADN_TRY(wpe_stream_state(c, wpe_state, wpe_state_bytes, n_slots / channels, n_fft / 2 + 1, channels, k));
    ADN_LAUNCH(adn::launch_wpe_mc_stream_pool(static_cast<float *>(pstate), y, channels, p.g, t, k, static_cast<float *>(wpe_state),
                                              static_cast<hipStream_t>(stream)), c.name);
    return ADN_OK;
}

static const char *resample_stream_text =": rates must be >= 1 with max(up, down) <= 4096 after dividing by their gcd, and at most "
                                          "16384 carried samples (2 floor(half / up) + ceil(down / up) + 1)";

static bool resample_stream_plan_ok(int src_rate, int dst_rate, adn::ResampleStreamGeom *g)
{
    return adn::resample_stream_geom(src_rate, dst_rate, g) && g->H <= adn::ADN_RESAMPLE_STREAM_MAX_H;
}

int adn_resample_stream_plan(int src_rate, int dst_rate, long received, int final, long *emitted, long *history, long *latency)
{
    adn::ResampleStreamGeom g;
    if (!resample_stream_plan_ok(src_rate, dst_rate, &g)) return fail(ADN_ERR_INVALID, std::string("adn_resample_stream_plan") + resample_stream_text);
    if (received < 0 || received >= (1L << 40)) return fail(ADN_ERR_INVALID, "adn_resample_stream_plan: need 0 <= received < 2^40");
    if (final != 0 && final != 1) return fail(ADN_ERR_INVALID, "adn_resample_stream_plan: final must be 0 or 1");
    if (emitted) *emitted = adn::resample_stream_emitted(g, received, final != 0);
    if (history) *history = g.H;
    if (latency) *latency = g.latency;
    return ADN_OK;
}

int adn_resample_stream_state_bytes(int n_streams, int src_rate, int dst_rate, size_t *bytes)
{
    adn::ResampleStreamGeom g;
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_resample_stream_state_bytes: null pointer");
    if (n_streams < 1) return fail(ADN_ERR_INVALID, "adn_resample_stream_state_bytes: n_streams must be >= 1");
    if (!resample_stream_plan_ok(src_rate, dst_rate, &g)) return fail(ADN_ERR_INVALID, std::string("adn_resample_stream_state_bytes") + resample_stream_text);
    *bytes = (size_t)n_streams * 2 * (size_t)g.H * sizeof(float);
    return ADN_OK;
}

int adn_resample_stream(void *state, size_t state_bytes, const float *audio, long audio_stride, int n_streams, long call_index,
                        long received_before, long n_new, int final, int src_rate, int dst_rate, float *out, long out_stride,
                        void *stream)
{
    adn::ResampleStreamGeom g;
    if (!resample_stream_plan_ok(src_rate, dst_rate, &g)) return fail(ADN_ERR_INVALID, std::string("adn_resample_stream") + resample_stream_text);
    if (n_streams < 1) return fail(ADN_ERR_INVALID, "adn_resample_stream: n_streams must be >= 1");
    if (final != 0 && final != 1) return fail(ADN_ERR_INVALID, "adn_resample_stream: final must be 0 or 1");
    if (n_new < (final ? 0 : 1)) return fail(ADN_ERR_INVALID, "adn_resample_stream: need n_new >= 1 (>= 0 in the final call)");
    if (call_index < 0 || received_before < 0 || (call_index == 0) != (received_before == 0))
        return fail(ADN_ERR_INVALID, "adn_resample_stream: need call_index >= 0 and received_before >= 0, both 0 in the first call of a stream and only there");
    if (received_before >= (1L << 31) || n_new >= (1L << 31) || received_before + n_new >= (1L << 31))
        return fail(ADN_ERR_INVALID, "adn_resample_stream: input positions must be < 2^31; end the stream before");
    const long m0 = adn::resample_stream_emitted(g, received_before, false);
    const long m1 = adn::resample_stream_emitted(g, received_before + n_new, final != 0);
    if (m1 >= (1L << 31)) return fail(ADN_ERR_INVALID, "adn_resample_stream: output positions must be < 2^31; end the stream before");
    const long n_out = m1 - m0;
    const bool copy = g.up == g.down;
    if ((!state && !copy) || (!audio && n_new > 0) || (!out && n_out > 0)) return fail(ADN_ERR_INVALID, "adn_resample_stream: null pointer");
    if (audio_stride < 0 || (n_streams > 1 && audio_stride < n_new))
        return fail(ADN_ERR_INVALID, "adn_resample_stream: audio_stride is smaller than n_new");
    if (out_stride < 0 || (n_streams > 1 && out_stride < n_out))
        return fail(ADN_ERR_INVALID, "adn_resample_stream: out_stride is smaller than the samples the call emits");
    if (!aligned_to(state, 8) || !aligned_to(audio, 4) || !aligned_to(out, 4))
        return fail(ADN_ERR_INVALID, "adn_resample_stream: state must be 8-byte aligned, audio and out 4-byte aligned");
    if (state_bytes < (size_t)n_streams * 2 * (size_t)g.H * sizeof(float))
        return fail(ADN_ERR_WORKSPACE, "adn_resample_stream: state smaller than adn_resample_stream_state_bytes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (copy) {                                           // equal rates: no filter, no state
        if (n_new > 0)
            ADN_HIP(hipMemcpy2DAsync(out, (size_t)(n_streams > 1 ? out_stride : n_new) * sizeof(float), audio,
                                     (size_t)(n_streams > 1 ? audio_stride : n_new) * sizeof(float), (size_t)n_new * sizeof(float),
                                     (size_t)n_streams, hipMemcpyDeviceToDevice, st));
        return ADN_OK;
    }
    hipError_t e = adn::launch_resample_stream(static_cast<float *>(state), audio, audio_stride, n_streams, g, call_index,
                                               received_before, n_new, final != 0, out, out_stride, st);
    if (e == adn::ADN_COLD_IN_CAPTURE)
        return fail(ADN_ERR_INVALID, "adn_resample_stream: first use of this (device, rate pair) on a stream that is being captured -- the "
                    "coefficient table is built with a blocking upload; call adn_resample_prepare(device, src_rate, dst_rate) before "
                    "the capture");
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, "adn_resample_stream: grid too large (n_streams x output blocks >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, "adn_resample_stream");
    return ADN_OK;
}

/* ---- streaming beamformer: recursive covariances, one filter per refresh (adn.h, "beamform stream") ------------------------------ */
// The parameters of a call on `channels` channels (NULL = the defaults), refused outside their legal ranges.
static int mvdr_stream_consts(const char *who, int channels, const adn_mvdr_stream_params *params, adn::MvdrStreamConsts *k)
{
    const std::string w(who);
    if (channels < 1 || channels > 8) return fail(ADN_ERR_INVALID, w + ": need 1 <= channels <= 8");
    const adn_mvdr_stream_params defaults = {0, 1, 0.99f, 1e-3f, 1e-3f};
    const adn_mvdr_stream_params p = params ? *params : defaults;
    if (p.refresh < 1 || p.refresh > 64) return fail(ADN_ERR_INVALID, w + ": need 1 <= refresh <= 64");
    // written so that a NaN fails the test
    if (!(p.forget >= 0.9f && p.forget <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0.9 <= forget <= 1");
    ADN_TRY(mvdr_fields(w, channels, p.ref_channel, p.loading, p.mask_floor, &k->m));
    k->R = p.refresh;
    k->alpha = p.forget;
    return ADN_OK;
}

static size_t mvdr_stream_bytes(int n_slots, int n_bins, int channels)
{
    return (size_t)n_slots * (size_t)n_bins * (size_t)adn::mvdr_stream_record_floats(channels) * sizeof(float);
}

static int mvdr_stream_state(const std::string &w, const void *state, size_t state_bytes, int n_slots, int n_bins, int channels)
{
    if (!state) return fail(ADN_ERR_INVALID, w + ": null pointer (the MVDR state)");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    if (state_bytes < mvdr_stream_bytes(n_slots, n_bins, channels))
        return fail(ADN_ERR_WORKSPACE, w + ": the MVDR state is smaller than adn_mvdr_stream_state_bytes");
    if (!aligned_to(state, 8)) return fail(ADN_ERR_INVALID, w + ": the MVDR state must be 8-byte aligned");
    return ADN_OK;
}

int adn_mvdr_stream_state_bytes(int n_slots, int channels, int n_bins, const adn_mvdr_stream_params *params, size_t *bytes)
{
    const std::string w("adn_mvdr_stream_state_bytes");
    adn::MvdrStreamConsts k;
    if (!bytes) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    ADN_TRY(mvdr_stream_consts("adn_mvdr_stream_state_bytes", channels, params, &k));
    *bytes = mvdr_stream_bytes(n_slots, n_bins, channels);
    return ADN_OK;
}

int adn_mvdr_online(const float *spec, const float *mag, int mag_width, int mag_col0, int n_groups, int channels, int n_frames,
                    int n_bins, long first_frame, const adn_mvdr_stream_params *params, void *state, size_t state_bytes, int n_slots,
                    float *spec_out, float *mag_out, int width, int col0, void *stream)
{
    const std::string w("adn_mvdr_online");
    adn::MvdrStreamConsts k;
    if (!spec || !mag || !spec_out) return fail(ADN_ERR_INVALID, w + ": null pointer (spec, mag, spec_out)");
    if (n_groups < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, w + ": n_groups, n_frames and n_bins must be >= 1");
    if (first_frame < 0 || first_frame + n_frames >= (1L << 31))
        return fail(ADN_ERR_INVALID, w + ": need first_frame >= 0 and first_frame + n_frames < 2^31");
    ADN_TRY(mvdr_stream_consts("adn_mvdr_online", channels, params, &k));
    if ((long)n_groups * channels > 0x7fffffffL) return fail(ADN_ERR_INVALID, w + ": need n_groups * channels < 2^31");
    ADN_TRY(mvdr_stream_state(w, state, state_bytes, n_slots, n_bins, channels));
    if (n_groups > n_slots) return fail(ADN_ERR_INVALID, w + ": group i uses slot i: need n_groups <= n_slots");
    if (mag_col0 < 0 || mag_width < 1 || (long)mag_col0 + n_frames > mag_width)
        return fail(ADN_ERR_INVALID, w + ": need mag_col0 >= 0 and mag_col0 + n_frames <= mag_width");
    if (mag_out && (col0 < 0 || width < 1 || (long)col0 + n_frames > width))
        return fail(ADN_ERR_INVALID, w + ": need col0 >= 0 and col0 + n_frames <= width");
    if (!aligned_to(spec, 8) || !aligned_to(spec_out, 8) || !aligned_to(mag, 4) || !aligned_to(mag_out, 4))
        return fail(ADN_ERR_INVALID, w + ": spec and spec_out must be 8-byte aligned, mag and mag_out 4-byte aligned");
    const size_t cells = (size_t)n_groups * (size_t)n_bins;
    const auto overlap = [](const void *p, size_t np, const void *q, size_t nq) {
        const char *a = reinterpret_cast<const char *>(p), *b = reinterpret_cast<const char *>(q);
        return a < b + nq && b < a + np;
    };
    const size_t in_spec = cells * channels * n_frames * 2 * sizeof(float), out_spec = cells * n_frames * 2 * sizeof(float);
    const size_t in_mag = cells * channels * mag_width * sizeof(float), out_mag = mag_out ? cells * width * sizeof(float) : 0;
    const size_t st_bytes = mvdr_stream_bytes(n_slots, n_bins, channels);
    if (overlap(spec, in_spec, spec_out, out_spec) || overlap(mag, in_mag, spec_out, out_spec) || overlap(state, st_bytes, spec_out, out_spec))
        return fail(ADN_ERR_INVALID, w + ": spec_out may not overlap spec, mag or the state");
    if (overlap(spec, in_spec, state, st_bytes) || overlap(mag, in_mag, state, st_bytes))
        return fail(ADN_ERR_INVALID, w + ": the state may not overlap spec or mag");
    if (mag_out && (overlap(spec, in_spec, mag_out, out_mag) || overlap(mag, in_mag, mag_out, out_mag) ||
                    overlap(spec_out, out_spec, mag_out, out_mag) || overlap(state, st_bytes, mag_out, out_mag)))
        return fail(ADN_ERR_INVALID, w + ": mag_out may not overlap spec, mag, spec_out or the state");
    if (adn::mvdr_stream_grid(n_groups, channels, n_bins) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (n_groups x ceil(n_bins / bins per workgroup) >= 2^31)");
    ADN_LAUNCH(adn::launch_mvdr_online(spec, mag, mag_width, mag_col0, n_groups, channels, n_frames, n_bins, (int)first_frame, k,
                                       static_cast<float *>(state), spec_out, mag_out, width, col0, static_cast<hipStream_t>(stream)),
               "adn_mvdr_online");
    return ADN_OK;
}

int adn_mvdr_stream(void *sstate, size_t sstate_bytes, float *y, int n_streams, int channels, long first_step, int n_steps,
                    long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                    const adn_mvdr_stream_params *params, void *mvdr_state, size_t mvdr_state_bytes, void *stream)
{
    const std::string w("adn_mvdr_stream");
    adn::StreamGeom g;
    adn::StreamCall call;
    adn::MvdrStreamConsts k;
    ADN_TRY(stream_state("adn_mvdr_stream", sstate, sstate_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, &g));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    ADN_TRY(stream_call("adn_mvdr_stream", g, first_step, n_steps, final_length, &call));
    ADN_TRY(mvdr_stream_consts("adn_mvdr_stream", channels, params, &k));
    if (n_streams % channels) return fail(ADN_ERR_INVALID, w + ": n_streams must be a multiple of channels");
    ADN_TRY(mvdr_stream_state(w, mvdr_state, mvdr_state_bytes, n_streams / channels, n_fft / 2 + 1, channels));
    if (adn::mvdr_stream_grid(n_streams / channels, channels, n_fft / 2 + 1) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (n_groups x ceil(n_bins / bins per workgroup) >= 2^31)");
    ADN_LAUNCH(adn::launch_mvdr_stream(static_cast<float *>(sstate), y, n_streams, channels, g, call, k,
                                       static_cast<float *>(mvdr_state), static_cast<hipStream_t>(stream)), "adn_mvdr_stream");
    return ADN_OK;
}

int adn_mvdr_stream_pool(void *pstate, size_t pstate_bytes, int n_slots, int channels, int n_fft, int hop, int window, int block,
                         int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                         const adn_mvdr_stream_params *params, void *mvdr_state, size_t mvdr_state_bytes, void *stream)
{
    const char *who = "adn_mvdr_stream_pool";
    const std::string w(who);
    PoolState p;
    adn::StreamPoolRows t = {};
    adn::MvdrStreamConsts k;
    int max_new, max_span;
    long max_out;
    ADN_TRY(pool_state(who, pstate, pstate_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    ADN_TRY(pool_rows(who, p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out));
    ADN_TRY(mvdr_stream_consts(who, channels, params, &k));
    ADN_TRY(pool_recordings(who, n_slots, channels, rows, n_rows));
    ADN_TRY(mvdr_stream_state(w, mvdr_state, mvdr_state_bytes, n_slots / channels, n_fft / 2 + 1, channels));
    ADN_LAUNCH(adn::launch_mvdr_stream_pool(static_cast<float *>(pstate), y, channels, p.g, t, k, static_cast<float *>(mvdr_state),
                                            static_cast<hipStream_t>(stream)), who);
    return ADN_OK;
}

/* ---- stream pool at a rate: rows of adn_resample_stream calls, into the rings and back (adn.h, "stream pool at a rate") ---- */
static_assert(ADN_STREAM_POOL_RATE_MAX_ROWS == adn::STREAM_POOL_RATE_MAX_ROWS, "adn.h and adn_internal.h disagree about the rate rows");

static int rate_state_check(const char *who, const void *rate_state, size_t rate_state_bytes, int n_slots, int max_history)
{
    const std::string w(who);
    if (n_slots < 1 || n_slots > (1 << 20) || max_history < 0 || max_history > adn::ADN_RESAMPLE_STREAM_MAX_H)
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 0 <= max_history <= 16384");
    if (!rate_state && max_history > 0) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(rate_state, 8)) return fail(ADN_ERR_INVALID, w + ": rate_state must be 8-byte aligned");
    if (rate_state_bytes < (size_t)n_slots * 4 * (size_t)max_history * sizeof(float))
        return fail(ADN_ERR_WORKSPACE, w + ": rate state smaller than adn_stream_pool_rate_state_bytes");
    return ADN_OK;
}

// The rows of a call, each inside adn_resample_stream's limits; push: src = the row's rate, dst = work_rate, direction 0.
// max_new / max_out: the most samples a row reads / writes.
static int rate_rows(const char *who, bool push, int n_slots, int max_history, int work_rate, const adn_stream_pool_rate_row *rows,
                     int n_rows, adn::ResampleStreamRow *t, long *max_new, long *max_out)
{
    const std::string w(who);
    if (!rows) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_rows < 1 || n_rows > ADN_STREAM_POOL_RATE_MAX_ROWS)
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_rows <= ADN_STREAM_POOL_RATE_MAX_ROWS (call again for the rest)");
    *max_new = *max_out = 0;
    for (int i = 0; i < n_rows; ++i) {
        const adn_stream_pool_rate_row r = rows[i];
        adn::ResampleStreamRow &o = t[i];
        if (r.slot < 0 || r.slot >= n_slots) return fail(ADN_ERR_INVALID, w + ": a row's slot is outside [0, n_slots)");
        for (int j = 0; j < i; ++j)
            if (rows[j].slot == r.slot) return fail(ADN_ERR_INVALID, w + ": a (slot, direction) is named twice in one call");
        if (!resample_stream_plan_ok(push ? r.rate : work_rate, push ? work_rate : r.rate, &o.g)) return fail(ADN_ERR_INVALID, w + resample_stream_text);
        if (o.g.H > max_history) return fail(ADN_ERR_INVALID, w + ": a row's rate pair carries more samples than max_history");
        if (r.final != 0 && r.final != 1) return fail(ADN_ERR_INVALID, w + ": final must be 0 or 1");
        if (r.n_new < (r.final ? 0 : 1)) return fail(ADN_ERR_INVALID, w + ": need n_new >= 1 (>= 0 in the final call)");
        if (r.call_index < 0 || r.received_before < 0 || (r.call_index == 0) != (r.received_before == 0))
            return fail(ADN_ERR_INVALID, w + ": need call_index >= 0 and received_before >= 0, both 0 in the first call of a stream and only there");
        if (r.received_before >= (1L << 31) || r.n_new >= (1L << 31) || r.received_before + r.n_new >= (1L << 31))
            return fail(ADN_ERR_INVALID, w + ": input positions must be < 2^31; end the stream before");
        const long m0 = adn::resample_stream_emitted(o.g, r.received_before, false);
        const long m1 = adn::resample_stream_emitted(o.g, r.received_before + r.n_new, r.final != 0);
        if (m1 >= (1L << 31)) return fail(ADN_ERR_INVALID, w + ": output positions must be < 2^31; end the stream before");
        if (r.audio_offset < 0) return fail(ADN_ERR_INVALID, w + ": audio_offset must be >= 0");
        o.slot = r.slot, o.direction = push ? 0 : 1;
        o.call_index = r.call_index, o.received_before = r.received_before, o.n_new = r.n_new;
        o.src_off = r.audio_offset;
        o.final = r.final != 0;
        if (r.n_new > *max_new) *max_new = r.n_new;
        if (m1 - m0 > *max_out) *max_out = m1 - m0;
        if (push && m1 >= (1L << 30)) return fail(ADN_ERR_INVALID, w + ": a pool's stream holds fewer than 2^30 samples at the working rate");
    }
    return ADN_OK;
}

static int rate_launch(const char *who, hipError_t e)
{
    const std::string w(who);
    if (e == adn::ADN_COLD_IN_CAPTURE)
        return fail(ADN_ERR_INVALID, w + ": first use of a (device, rate pair) on a stream that is being captured -- the coefficient "
                    "table is built with a blocking upload; call adn_resample_prepare(device, src_rate, dst_rate) before the capture");
    if (e == hipErrorInvalidValue) return fail(ADN_ERR_INVALID, w + ": grid too large (output blocks >= 2^31)");
    if (e != hipSuccess) return fail_hip(e, who);
    return ADN_OK;
}

int adn_stream_pool_rate_state_bytes(int n_slots, int max_history, size_t *bytes)
{
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_stream_pool_rate_state_bytes: null pointer");
    if (n_slots < 1 || n_slots > (1 << 20) || max_history < 0 || max_history > adn::ADN_RESAMPLE_STREAM_MAX_H)
        return fail(ADN_ERR_INVALID, "adn_stream_pool_rate_state_bytes: need 1 <= n_slots <= 2^20 and 0 <= max_history <= 16384");
    *bytes = (size_t)n_slots * 4 * (size_t)max_history * sizeof(float);
    return ADN_OK;
}

int adn_stream_pool_push_rate(void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block, int lookahead,
                              long ring_samples, void *rate_state, size_t rate_state_bytes, int max_history, int work_rate,
                              const adn_stream_pool_rate_row *rows, int n_rows, const float *audio, void *stream)
{
    static const char *who = "adn_stream_pool_push_rate";
    PoolState p;
    adn::ResampleStreamRow t[ADN_STREAM_POOL_RATE_MAX_ROWS];
    long max_new, max_out;
    int rc = pool_state(who, state, state_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p);
    if (rc != ADN_OK) return rc;
    rc = rate_state_check(who, rate_state, rate_state_bytes, n_slots, max_history);
    if (rc != ADN_OK) return rc;
    rc = rate_rows(who, true, n_slots, max_history, work_rate, rows, n_rows, t, &max_new, &max_out);
    if (rc != ADN_OK) return rc;
    if (max_out > p.R) return fail(ADN_ERR_INVALID, "adn_stream_pool_push_rate: a row writes more samples than ring_samples");
    if (!audio && max_new > 0) return fail(ADN_ERR_INVALID, "adn_stream_pool_push_rate: null pointer");
    if (!aligned_to(audio, 4)) return fail(ADN_ERR_INVALID, "adn_stream_pool_push_rate: audio must be 4-byte aligned");
    return rate_launch(who, adn::launch_resample_stream_rows(t, n_rows, audio, static_cast<float *>(rate_state), max_history,
                                                             static_cast<float *>(state), 0, true, p.ring_off, p.R,
                                                             static_cast<hipStream_t>(stream)));
}

int adn_stream_pool_emit_rate(void *rate_state, size_t rate_state_bytes, int n_slots, int max_history, int work_rate,
                              const adn_stream_pool_rate_row *rows, int n_rows, const float *audio_in, long in_stride, float *out,
                              long out_stride, void *stream)
{
    static const char *who = "adn_stream_pool_emit_rate";
    adn::ResampleStreamRow t[ADN_STREAM_POOL_RATE_MAX_ROWS];
    long max_new, max_out;
    int rc = rate_state_check(who, rate_state, rate_state_bytes, n_slots, max_history);
    if (rc != ADN_OK) return rc;
    rc = rate_rows(who, false, n_slots, max_history, work_rate, rows, n_rows, t, &max_new, &max_out);
    if (rc != ADN_OK) return rc;
    if ((!audio_in && max_new > 0) || (!out && max_out > 0)) return fail(ADN_ERR_INVALID, "adn_stream_pool_emit_rate: null pointer");
    if (in_stride < 0 || (n_rows > 1 && in_stride < max_new))
        return fail(ADN_ERR_INVALID, "adn_stream_pool_emit_rate: in_stride is smaller than a row's n_new");
    if (out_stride < 0 || (n_rows > 1 && out_stride < max_out))
        return fail(ADN_ERR_INVALID, "adn_stream_pool_emit_rate: out_stride is smaller than the samples a row emits");
    if (!aligned_to(audio_in, 4) || !aligned_to(out, 4)) return fail(ADN_ERR_INVALID, "adn_stream_pool_emit_rate: audio_in and out must be 4-byte aligned");
    for (int i = 0; i < n_rows; ++i) t[i].src_off += (long)i * in_stride;
    return rate_launch(who, adn::launch_resample_stream_rows(t, n_rows, audio_in, static_cast<float *>(rate_state), max_history, out,
                                                             out_stride, false, 0, 0, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
