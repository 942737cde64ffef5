/* e2etts_critic.h -- C ABI of the vocoder-critic companion library (libe2etts_critic.so).
 *
 * The eval() forward of HiFi-GAN's multi-period and multi-scale discriminators (reference V/discriminator.py, V/layers.py:72-133) on the
 * GPU, and the figures of V/loss.py on their outputs: feature_loss, discriminator_loss, generator_loss.  Forward and loss VALUES only: no
 * backward pass, no optimiser.  All arithmetic is exact fp32; the figures are reduced in double.  THE DEFINITION BELOW IS THE CONTRACT.
 *
 * Definition.
 *   rows     a batch is B rows of samples, row b with lens[b] samples, E2ECR_MIN_LEN <= lens[b] <= ld (the row stride).  The reference
 *            takes dense [B, 1, T] and knows no lengths; here EVERY ROW IS EVALUATED OVER ITS OWN LENGTH, as its own B = 1 call would be
 *            (the reflect extension, every layer's zero padding at the row's own end, the pooling), every figure is per row, and every
 *            row equals its B = 1 call bit for bit whatever the batch, the grid and the tile are.  For a batch of equal lengths the mean
 *            of the per-row figures is the reference's batch figure up to rounding.
 *   lengths  the output length of every convolution is floor((n + 2 pad - k) / stride) + 1 over the row's own input length n.
 *   period   discriminator p: a row of n samples is extended at its end by p - n % p reflected samples when n % p != 0 (F.pad(mode =
 *            "reflect"): sample n + m is sample n - 2 - m, the edge sample is not repeated), then folded to [H = ceil(n / p), p]; each of
 *            the p columns is an independent 1-D sequence.  n_mpd_layers convolutions (Cin of the first is 1), each followed by leaky
 *            ReLU (v >= 0 ? v : v * slope); THE FEATURE MAP IS THE ACTIVATED OUTPUT.  Then mpd_post (Cout 1, stride 1) without activation:
 *            its output is the last feature map and, flattened (h major, column minor), the score.
 *   scale    discriminator i of n_scales sees the row after i applications of AvgPool1d(4, 2, padding = 2): out[t] = (((x[2t - 2] +
 *            x[2t - 1]) + x[2t]) + x[2t + 1]) * 0.25 in double, rounded once, with zeros outside [0, n) (the divisor is 4 whatever the padding covers), n / 2 + 1
 *            outputs.  n_msd_layers convolutions with groups, leaky ReLU after each, then msd_post.
 *   order    every map element is float32.  First layers, the pool and *_post sum in double -- the product of two floats is exact there --
 *            and round once after the bias (a score is a sum of 3 C terms that largely cancel): first layers taps ascending; post: per
 *            lane of 64 the channels lane, lane + 64, ... within tap 0, 1, ..., the lanes'
 *            sums merged by a fixed xor tree 32, 16, ... 1.  Grouped and dense layers sum fp32 fused multiply-adds from 0, add the bias,
 *            then activate.  Grouped layers: four chains per element, tap j in chain j % 4, within a
 *            chain taps ascending and the group's input channels ascending within a tap, merged (c0 + c1) + (c2 + c3) before the bias.
 *            Dense layers (groups 1, Cin > 1): the folded channel axis is cut into n <= 8 equal ranges (csrc/critic/plan.h: dense_splits);
 *            per range one chain in the order of this project's exact-fp32 conv_gemm on the stride-folded weights (32-channel chunks,
 *            then folded tap, then channel); the ranges' sums merged by the tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)),
 *            then the bias.  A single chain of K = 5120 terms carries a rounding error that grows like K; the split keeps it near 1 / sqrt(n).
 *   figures  per row, in double.  A mean over N values v_e (e in the order [column, position, channel] of the map): value e goes to lane
 *            e % 256 of chunk e / 4096; a lane adds its up to 16 values in ascending e; the 256 lanes of a chunk are merged by the tree
 *            v[i] += v[i + s], s = 128, 64, ... 1; the chunks' sums go to lane (chunk % 256) in ascending order and the lanes are merged by
 *            the same tree; the sum is divided by N.  No atomics: the same bits from run to run.
 *              fm[d][l]   = mean |double(r) - double(g)| over layer l's map of discriminator d (discriminators: the periods in the config's
 *                           order, then the scales), l = n_layers for the post map;
 *              d_real[d]  = mean (1 - D(y))^2,  d_fake[d] = mean D(g)^2,  g_fake[d] = mean (1 - D(g))^2 over the row's scores;
 *              feature_loss_* = 2 * (sum of fm in d, l order), disc_loss_* = sum_d (d_real + d_fake), gen_loss_* = sum_d g_fake, summed
 *                           on the host in double in that order, separately over the period and the scale discriminators.
 *            The feature distance needs y_lens[b] == g_lens[b]: a row where they differ gets E2ECR_ST_LENGTHS_DIFFER, its score figures,
 *            and NaN in fm and feature_loss_*; the other rows are untouched.  A one-sided call (g == NULL) computes the scores of y
 *            alone: d_real = mean (1 - D(y))^2, d_fake = mean D(y)^2, g_fake = d_real, fm NaN, status E2ECR_ST_ONE_SIDED.
 *   calls    e2ecr_run is the fused call: both sides go through as one batch of 2 B rows, every layer's figures are reduced right after
 *            the layer, the maps live in two alternating buffers and are never kept.  Above the workspace cap of the config the batch is
 *            processed in groups of pairs, which changes no bit.  e2ecr_forward is the materialising call for ONE side: every map stays
 *            resident until the next call and e2ecr_fetch_fmap hands it out in the reference's layout.  The figures of e2ecr_run equal
 *            the figures computed from e2ecr_forward's maps by the reduction above, bit for bit.
 *   weights  e2ecr_load_weights takes a blob of packer.pack_critic (build_blob's container): per discriminator and layer the effective
 *            fp32 weights (weight_norm / spectral_norm folded by the packer), the dense strided layers already stride-folded, the grouped
 *            layers in MFMA-fragment order.
 *
 * Layer support.  groups == 1 with Cin > 1: any stride (folded), Cin % 4 == 0.  groups > 1: Cin / groups a multiple of 8, Cout / groups a
 * multiple of 16, and the staged input window of a tile must fit 64 KiB of LDS.  Anything else is refused by name at e2ecr_create.
 *
 * Conventions: those of e2etts_compare.h (plain C; 0 or a negative E2ECR_E* code, e2ecr_last_error() has the message; data pointers may
 * be host or device memory; lengths are int64 HOST OR DEVICE arrays read during validation; every argument is validated before anything is
 * enqueued; the handle works on its own stream and every computing call returns after it has drained; e2ecr_order_after orders it after
 * a caller's stream, so a vocoder's resident output needs no visit to the host; workspaces grow and never shrink; one thread at a time).
 *
 * Exports: 17 entry points, and 2 more in the test build.
 */
#ifndef E2ETTS_CRITIC_H
#define E2ETTS_CRITIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2ECR_API __attribute__((visibility("default")))
#else
#define E2ECR_API
#endif

#define E2ECR_ABI_VERSION 1

#define E2ECR_OK 0
#define E2ECR_EINVAL (-1)
#define E2ECR_EHIP (-2)
#define E2ECR_ESTATE (-3)
#define E2ECR_ENOMEM (-4)

#define E2ECR_MAX_B 4096
#define E2ECR_MAX_LEN (1 << 24)   /* samples per row */
#define E2ECR_MIN_LEN 12          /* the largest period + 1 of the default config: the reflect extension of period 11 needs 11 samples
                                     before the edge.  A config's own minimum is max(periods) + 1 (at least 2). */
#define E2ECR_MAX_PERIODS 8
#define E2ECR_MAX_SCALES 4
#define E2ECR_MAX_LAYERS 8        /* convolutions before *_post */
#define E2ECR_MAX_DISC (E2ECR_MAX_PERIODS + E2ECR_MAX_SCALES)
#define E2ECR_MAX_MAPS (E2ECR_MAX_LAYERS + 1)

#define E2ECR_F32 0     /* samples fp32 in [-1, 1] */
#define E2ECR_PCM16 1   /* int16 PCM: sample / 32768 (exact in fp32) */

#define E2ECR_ST_LENGTHS_DIFFER 1
#define E2ECR_ST_ONE_SIDED 2

typedef struct e2ecr_handle e2ecr_handle;

typedef struct e2ecr_layer {
  int32_t cout, k, stride, groups, pad;
} e2ecr_layer;

/* The layer tables.  Cin of a first layer is 1, Cin of a later one the Cout before it; *_post has cout 1, stride 1, groups 1. */
typedef struct e2ecr_config {
  int32_t n_periods;
  int32_t periods[E2ECR_MAX_PERIODS];
  int32_t n_mpd_layers;
  e2ecr_layer mpd[E2ECR_MAX_LAYERS];   /* groups 1 */
  e2ecr_layer mpd_post;
  int32_t n_scales;
  int32_t n_msd_layers;
  e2ecr_layer msd[E2ECR_MAX_LAYERS];
  e2ecr_layer msd_post;
  float slope;                         /* leaky ReLU */
  int32_t reserved;
  int64_t workspace_cap_bytes;         /* the two alternating map buffers and the dense layers' partial sums together; 0: 2 GiB */
} e2ecr_config;

/* One row's figures: int64 and double only.  Unused entries are NaN. */
typedef struct e2ecr_result {
  int64_t status;
  int64_t n_disc;
  double fm[E2ECR_MAX_DISC][E2ECR_MAX_MAPS];
  double d_real[E2ECR_MAX_DISC], d_fake[E2ECR_MAX_DISC], g_fake[E2ECR_MAX_DISC];
  double feature_loss_mpd, feature_loss_msd;
  double disc_loss_mpd, disc_loss_msd;
  double gen_loss_mpd, gen_loss_msd;
} e2ecr_result;

E2ECR_API const char* e2ecr_version(void);
E2ECR_API int e2ecr_abi_version(void);
E2ECR_API const char* e2ecr_last_error(const e2ecr_handle* handle);

/* The reference's tables: periods 2, 3, 5, 7, 11; 3 scales; slope 0.1. */
E2ECR_API void e2ecr_default_config(e2ecr_config* out);
/* config == NULL: the default.  Opens no device. */
E2ECR_API int e2ecr_create(int device_id, const e2ecr_config* config, e2ecr_handle** out);
E2ECR_API void e2ecr_destroy(e2ecr_handle* handle);
E2ECR_API int e2ecr_load_weights(e2ecr_handle* handle, const void* blob, size_t nbytes);

E2ECR_API void* e2ecr_stream(e2ecr_handle* handle);
E2ECR_API int e2ecr_order_after(e2ecr_handle* handle, void* caller_stream);
E2ECR_API int e2ecr_sync(e2ecr_handle* handle);
E2ECR_API size_t e2ecr_device_bytes(const e2ecr_handle* handle);

/* The fused call.  y [B, ld_y] and g [B, ld_g] samples of `dtype`, each side with a row stride of its own (a recording and a vocoder's
 * output seldom share one); g may be NULL: one-sided, ld_g is then ignored; y_lens, g_lens [B] int64; results_out [B] (host). */
E2ECR_API int e2ecr_run(e2ecr_handle* handle, const void* y, const int64_t* y_lens, long long ld_y, const void* g, const int64_t* g_lens, long long ld_g, int B,
                        int dtype, e2ecr_result* results_out);
/* The raw scores of the last e2ecr_run / e2ecr_forward: side 0 = y (or the forward's batch), 1 = g; out [B, n_max] fp32, row b holds its
 * n[b] scores followed by zeros; n_out [B] (host, may be NULL); out may be NULL to ask for the sizes: *n_max_out is the row length. */
E2ECR_API int e2ecr_fetch_scores(e2ecr_handle* handle, int side, int disc, float* out, long long* n_out, long long* n_max_out);

/* The materialising call for one batch: every map of every discriminator stays resident until the next computing call. */
E2ECR_API int e2ecr_forward(e2ecr_handle* handle, const void* x, const int64_t* lens, int B, long long ld, int dtype);
/* Map `layer` (n_layers: the post map) of discriminator `disc` of the last e2ecr_forward in the reference's layout: [B, C, Tmax, p] for a
 * period discriminator, [B, C, Tmax] for a scale discriminator, fp32, zeros at t >= t_out[b].  shape_out [4] (B, C, Tmax, p or 1) and
 * t_out [B] are host arrays (may be NULL); out may be NULL to ask for the shape. */
E2ECR_API int e2ecr_fetch_fmap(e2ecr_handle* handle, int disc, int layer, float* out, long long* shape_out, long long* t_out);

/* With profiling on, e2ecr_profile_read gives the last e2ecr_run's milliseconds as {dense (conv_gemm) layers, grouped layers, everything
 * else: first layers, pool, post, reductions} from HIP events around every launch (which serialises nothing: one stream). */
E2ECR_API int e2ecr_profile_enable(e2ecr_handle* handle, int on);
E2ECR_API int e2ecr_profile_read(e2ecr_handle* handle, double ms_out[3]);

#ifdef E2ECR_TEST_HOOKS
/* Test build only (libe2etts_critic_test.so). */
E2ECR_API int e2ecr_debug_poison_workspace(e2ecr_handle* handle);
/* The grouped convolution kernel alone on DEVICE buffers of the caller: in [B, t_in_cap, cin] channels-last, lens_in [B] int32 device,
 * wfrag in the packer's fragment order, bias [cout], out [B, t_out_cap, cout]: rows t < out_len(lens_in[b]) hold the result, rows up to
 * t_out_cap are written as 0.  tm: 0 for the plan's tile, or a tile to force (a multiple of 64). */
E2ECR_API int e2ecr_debug_grouped_conv(e2ecr_handle* handle, const float* in, const int32_t* lens_in, const float* wfrag, const float* bias, float* out, int B,
                                       int t_in_cap, int t_out_cap, int cin, int cout, int k, int stride, int groups, int pad, float slope, int tm);
#endif

#ifdef __cplusplus
}
#endif
#endif
