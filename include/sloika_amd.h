/*
 * sloika_amd.h -- C ABI of the MI355X (gfx950) basecalling hot path.
 *
 * Drop-in boundary for ONE path of nanoporetech/sloika:
 *     chunkify/normalise -> conv front end -> stacked GRU/LSTM -> softmax -> k-mer Viterbi decode
 *     (+ the transducer remap DP).
 * The reference implements this path in Python/numpy on top of Theano-generated code plus one Cython
 * function; each entry point below names the reference interface (file:line, relative to the sloika
 * checkout) it replaces.  INTEGRATION.md shows the binding a sloika maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - ALL pointers are DEVICE pointers (HIP) unless the parameter is documented as host.
 *     The library never allocates, frees or synchronises; scratch space is passed in by the caller
 *     (size from the matching *_workspace_bytes function).
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*; NULL = the null stream)
 *     and returns immediately.  Safe to capture into a hipGraph.
 *   - return value: SLK_OK (0) or a negative SLK_ERR_* code; nothing throws.
 *   - tensors are float32, C order [time][batch][feature] (sloika/layers.py:13-14).
 *   - thread-safe and re-entrant: no global state.
 */
#ifndef SLOIKA_AMD_H
#define SLOIKA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLK_ABI_VERSION 1
/* Every entry point below is exported; nothing else in libsloika_amd.so is (the library is built with
 * -fvisibility=hidden, tests/test_cabi.py compares the export table with this header both ways).          */
#define SLK_API __attribute__((visibility("default")))

#define SLK_OK 0
#define SLK_ERR_INVALID_ARG (-1) /* bad shape / null pointer: the reference raises AssertionError here      */
#define SLK_ERR_UNSUPPORTED (-2) /* valid request this build has no kernel for                               */
#define SLK_ERR_LAUNCH (-3)      /* HIP reported a launch error                                              */
#define SLK_ERR_WORKSPACE (-4)   /* workspace pointer null or too small                                      */
#define SLK_ERR_NO_DEVICE (-5)   /* no HIP device visible to this process                                    */

/* Activation ids: one per function of sloika/activation.py:8-115 (same order as the file).                  */
enum slk_activation {
    SLK_ACT_LINEAR = 0,      /* activation.py:8   */
    SLK_ACT_TANH = 1,        /* activation.py:52  */
    SLK_ACT_SIGMOID = 2,     /* activation.py:56  */
    SLK_ACT_ELU = 3,         /* activation.py:38  */
    SLK_ACT_RELU = 4,        /* activation.py:12  */
    SLK_ACT_RELU_SMOOTH = 5, /* activation.py:16  */
    SLK_ACT_SOFTPLUS = 6,    /* activation.py:21  */
    SLK_ACT_EXP = 7,         /* activation.py:45  */
    SLK_ACT_ERF = 8,         /* activation.py:60  */
    SLK_ACT_L1ML2 = 9,       /* activation.py:64  */
    SLK_ACT_FAIR = 10,       /* activation.py:68  */
    SLK_ACT_RETU = 11,       /* activation.py:72  */
    SLK_ACT_TANH_PM = 12,    /* activation.py:81  */
    SLK_ACT_SIGMOID_PM = 13, /* activation.py:88  */
    SLK_ACT_BOUNDED_LINEAR = 14, /* activation.py:95 */
    SLK_ACT_SIN = 15,        /* activation.py:102 */
    SLK_ACT_CAUCHY = 16,     /* activation.py:106 */
    SLK_ACT_GEMAN_MCCLURE = 17, /* activation.py:110 */
    SLK_ACT_WELSH = 18,      /* activation.py:114 */
    SLK_ACT_COUNT = 19
};

typedef void *slk_stream_t; /* hipStream_t */

SLK_API int slk_abi_version(void);
SLK_API const char *slk_error_string(int code);
/* Number of HIP devices visible (host call; does not create a context when 0).                               */
SLK_API int slk_device_count(void);
/* Device self-test: one v_mfma_f32_4x4x1_16b_f32 on 64 lanes, a[lane], b[lane] -> d[4][64], with the CBSZ / ABID broadcast
 * modifiers the exact-fp32 recurrent kernels rely on (cbsz, abid in {(0,0), (4,0), (4,3), (4,15), (3,0), (3,5), (2,1), (2,3)}):
 * lets an integrator confirm on the installed device the operand layout those kernels assume.                              */
/* Measurement aid: the shader clock the device holds at the moment the probe runs.  One wave reads the shader-cycle counter and
 * the constant 100 MHz counter around `spins` x 127 sleep quanta; out2[0] / out2[1] x 100 = MHz (device memory, two uint64).
 * Launched on a stream of its own beside a running workload it reports the clock under that load (bench.py `sustained`).     */
SLK_API int slk_clock_probe(unsigned long long *out2, int spins, slk_stream_t stream);
SLK_API int slk_selftest_mfma4_f32(const float *a, const float *b, float *d, int cbsz, int abid, slk_stream_t stream);

/* Elementwise activation y[i] = act(x[i]) (sloika/activation.py); in place allowed (y == x).                 */
SLK_API int slk_activation_f32(const float *x, float *y, size_t count, int act, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a1. Chunk front end: per-chunk median/MAD normalisation.
 * Replaces: sloika/tools/chunkify_raw.py:172-181 ("per-chunk" branch of raw_chunkify), the same maths as
 * sloika/basecall.py:117-118 and sloika/maths.py:4-27 (factor 1.4826, numpy median semantics).
 *   signal : [nchunk][chunk_len] float32 (chunk-major, as raw_chunkify's reshape produces it)
 *   out    : element (c, i) is written at out[c*out_chunk_stride + i*out_sample_stride]
 *            (out_chunk_stride=chunk_len, out_sample_stride=1 keeps chunk-major;
 *             out_chunk_stride=1, out_sample_stride=nchunk writes the [T][B][1] network layout of
 *             bin/train_network.py:304 directly)
 *   med_out, mad_out : optional [nchunk] (NULL to skip); mad includes the 1.4826 factor.
 * Results are bit-identical to numpy's float32 evaluation.  Any chunk_len (LDS sort up to 32768 samples, exact radix
 * selection beyond: whole reads).  -0.0 and +0.0 are distinct keys in the selection; NaNs are not supported.
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_med_mad_normalise_f32(const float *signal, int nchunk, int chunk_len, float *out,
                              long out_chunk_stride, long out_sample_stride, float *med_out, float *mad_out,
                              slk_stream_t stream);
/* The same per READ for a batch of whole reads of different lengths (sloika/basecall.py:117-118 normalises a read over its own
 * length): read r is lens[r] samples at signal + r*in_stride; element (r, i), i < lens[r], goes to
 * out[r*out_chunk_stride + i*out_sample_stride]; nothing else is written (the caller zero-fills a padded batch) and nothing
 * behind lens[r] is read.  A read with lens[r] <= 0 is skipped: none of its outputs is written, med_out[r] and mad_out[r] included.
 * Exact order statistics by radix selection, any length >= 1; bit-identical to slk_med_mad_normalise_f32 on each read alone. */
SLK_API int slk_med_mad_normalise_ragged_f32(const float *signal, int nread, long in_stride, const int32_t *lens, float *out,
                                             long out_chunk_stride, long out_sample_stride, float *med_out, float *mad_out,
                                             slk_stream_t stream);
/* Whole-read mode (sloika/basecall.py:88-121 calls reads one at a time; the build batches reads of similar length): the read set lies
 * in one device buffer, read r in src[start[r] .. start[r] + len[r]).
 *   slk_pack_reads_f32       dst:[nread][ld] (ld >= max len) <- the reads, zero-padded to ld samples each
 *   slk_reads_nonfinite_f32  flags[r] |= 1 when read r holds a NaN or an infinity (flags zeroed by the caller; max_len >= max len):
 *                            such a read is skipped and reported, as raw_worker skips a read that fails (basecall.py:103-115),
 *                            instead of poisoning the batch it would have shared.                                               */
SLK_API int slk_pack_reads_f32(const float *src, const int64_t *start, const int32_t *len, int nread, float *dst, long ld,
                       slk_stream_t stream);
SLK_API int slk_reads_nonfinite_f32(const float *src, const int64_t *start, const int32_t *len, int nread, int max_len, int32_t *flags,
                            slk_stream_t stream);
/* int16 ADC samples -> float32 picoamperes on the device, what sloika/basecall.py:105 (fast5 get_read(raw=True)) and the float32 cast of
 * the float flows do on the host: (float)(((double)adc + offset[r]) * scale[r]), a double add, a double multiply and one round to
 * float -- bit for bit numpy's ((adc.astype(float64) + offset) * (range / digitisation)).astype(float32) when the caller computes
 * scale[r] = (double)range / (double)digitisation.  Read r: src[start[r] .. start[r] + len[r]) -> dst at the same indices, and
 * dst[start[r] + len[r] .. start[r] + stride[r]) = +0.0f (len[r] <= stride[r]); nothing else is written.  flags (nullable, zeroed by the
 * caller): flags[r] |= 1 when an output sample of read r is not finite (slk_reads_nonfinite_f32's check, in the same pass).  All arrays
 * are device arrays of nread entries; max_stride >= every stride[r] sizes the grid.  Any nread and any start (a start that leaves the
 * input and output offsets unequal mod 4 samples takes a scalar path).                                                              */
SLK_API int slk_adc_to_pa_i16(const int16_t *src, const int64_t *start, const int32_t *len, const int32_t *stride, const double *offset,
                              const double *scale, int nread, int max_stride, float *dst, int32_t *flags, slk_stream_t stream);
/* batch.trim_open_pore(signal, max_op_fraction=0) + util.trim_array for every read of an uploaded set, without a round trip to the host
 * (sloika/batch.py:194-220 with the CLI's default fraction, bin/basecall_network.py:71: np.percentile(., 0) is the minimum; then
 * sloika/basecall.py:111-112).  spread: the per-window spreads of ALL reads (MAD or std of every `window` samples, as
 * slk_med_mad_normalise_f32 / slk_window_std_f32 leave them); read r owns windows first_win[r] .. first_win[r] + nwin[r] (whole windows
 * only, as the reference's reshape) and starts at sample first_sample[r] of the set.  Out: start[r] (sample index in the set) and len[r]
 * of the trimmed read.  flags[r]: bit 0 set by the caller = the read holds a sample that is not finite; on return bit 1 = the reference's
 * function fails on the read (no whole window, or no window livelier than the minimum), bit 2 = nothing left after trimming; a read with
 * any bit set gets len 0 (the reference's worker reports it and goes on, sloika/basecall.py:103-115).                              */
SLK_API int slk_open_pore_trim_f32(const float *spread, const int64_t *first_win, const int32_t *nwin, const int64_t *first_sample,
                           int nread, int window, int trim0, int trim1, int64_t *start, int32_t *len, int32_t *flags,
                           slk_stream_t stream);
/* Standard deviation of each of nwin consecutive windows of `win` samples (population form, numpy's .std()):
 * batch.trim_open_pore(var_method='std'), sloika/batch.py:210-211.  out:[nwin].                                    */
SLK_API int slk_window_std_f32(const float *signal, int nwin, int win, float *out, slk_stream_t stream);
/* a1 for the event models: features.from_events (sloika/features.py:6-32) with maths.studentise (sloika/maths.py:48-58) for a ragged
 * set of `nseg` segments in one launch.  mean, stdv, length: the event table's columns, all three float32 (columns_f64 == 0) or all
 * three float64 (columns_f64 != 0).  Segment s is the events seg_start[s] .. seg_start[s] + seg_len[s] - 1: a whole read, or one
 * chunk's window of a read (batch.chunkify 'per-chunk', sloika/batch.py:37-49).  Its rows are
 *     [mean, stdv, length, |mean[e+1] - mean[e]|]   as float32, the last row's fourth column 0 (features.py:17-22);
 * with `normalise` every column is studentised over the WHOLE segment (population standard deviation, one that is not > 0 replaced
 * by 1); with `nanonet` the fourth column is the signed delta over its own standard deviation instead (features.py:27-30).  Only the
 * first seg_keep[s] rows are written (seg_keep[s] > seg_len[s] counts as seg_len[s]): row i, column c of segment s goes to
 *     out[4 * out_row[s] + i * ld_out + c]
 * (ld_out = 4 and out_row = the segment's first row for a dense [rows][4] matrix; ld_out = 4 * B and out_row = b for column b of a
 * [T][B][4] network input).  ld_out is a multiple of 4 and `out` 16-byte aligned: a row is one 16-byte store.  Nothing else is
 * written.  Moments are accumulated in float64 in an order that depends on the segment alone, the result is rounded to float32 once:
 * a segment gets the same bits whatever shares the launch.  Any seg_len >= 1 (a segment of length 0 writes nothing), nseg < 2^31. */
SLK_API int slk_event_features_f32(const void *mean, const void *stdv, const void *length, int columns_f64, const int64_t *seg_start,
                                   const int64_t *seg_len, const int64_t *seg_keep, int64_t nseg, int normalise, int nanonet,
                                   float *out, const int64_t *out_row, int64_t ld_out, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a3. Convolution.run  (sloika/layers.py:417-419 -> sloika/conv.py:66-77,90-111)
 *   y[to][b][o] = act( sum_{c,k} xpad[to*stride + k][b][c] * W[o][c][k] + bias[o] ), zero padding
 *   (pad_l, pad_r) on the time axis, cross-correlation (filter_flip=False).
 *   x : element (t, b, c) at x[t*x_t_stride + b*x_b_stride + c]   (x_t_stride=B*Cin, x_b_stride=Cin for the
 *       reference layout; x_t_stride=1, x_b_stride=T reads chunk-major signal when Cin == 1)
 *   W : [Cout][Cin][winlen]   bias: [Cout] or NULL   y : [Tout][B][Cout], Tout = slk_conv1d_out_len(...)
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_conv1d_out_len(int T, int winlen, int stride, int pad_l, int pad_r);
SLK_API int slk_conv1d_f32(const float *x, long x_t_stride, long x_b_stride, const float *W, const float *bias, float *y,
                   int T, int B, int Cin, int Cout, int winlen, int stride, int pad_l, int pad_r, int act,
                   slk_stream_t stream);

/* a3b. Window.run (sloika/layers.py:346-351): zero pad w/2 both ends, y[t][b][k*F+f] = xpad[t+k][b][f].      */
SLK_API int slk_window_f32(const float *x, float *y, int T, int B, int F, int w, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a6. FeedForward.run (sloika/layers.py:157-158) and every other `tensordot(x, W, axes=(2,1)) + b`:
 *   y[r][j] = act( sum_k x[r][k] * W[j][k] + bias[j] ),  r < M (= T*B rows), j < N, k < K.
 *   x rows are ldx floats apart, y rows ldy floats apart (lets Parallel/birnn outputs be written straight
 *   into their slice of the concatenated tensor, sloika/layers.py:1486-1487).  W:[N][K] dense.  fp32 MFMA.
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_gemm_bias_act_f32(const float *x, long ldx, const float *W, const float *bias, float *y, long ldy,
                          long M, int K, int N, int act, slk_stream_t stream);

/* Softmax.run (sloika/layers.py:309-314): logits = x.W^T + b; p = exp(l - max) / sum.  y:[M][N] dense.      */
SLK_API int slk_linear_softmax_f32(const float *x, long ldx, const float *W, const float *bias, float *y, long M, int K,
                           int N, slk_stream_t stream);
/* x-stationary variant for wide outputs (csrc/gemm_rows.hip): logits y[r][j] = x[r].W[j] + b[j] with row stride ldy,
 * plus (when stats != NULL) stats[r] = (max_j, 1 / sum_j exp(y[r][j] - max_j)) accumulated on the fly.  K <= 128, else
 * SLK_ERR_UNSUPPORTED.  slk_softmax_from_stats_f32 turns (logits, stats) into the posterior exp(l - max) * inv_sum.    */
SLK_API int slk_linear_rowstats_f32(const float *x, long ldx, const float *W, const float *bias, float *y, long ldy, long M, int K,
                            int N, float *stats /* [M][2] or NULL */, slk_stream_t stream);
SLK_API int slk_softmax_from_stats_f32(const float *logits, long ld_in, const float *stats, float *post, long ld_out, long M,
                               int N, slk_stream_t stream);
/* Same contraction on the FP16 matrix pipe with float32-grade accuracy (csrc/gemm_rows_f16x3.hip): operands split
 * v = hi + lo in fp16, x.w ~= x_hi.w_hi + x_hi.w_lo + x_lo.w_hi accumulated in float32 -- ~5x the fp32-MFMA
 * throughput, error a few float32 ulps.  Weights are split once with slk_split_f16x2_f32 into two fp16 matrices
 * [N][KP], KP = K rounded up to 16 (2*N*KP bytes each), every row scaled by a power of two that brings its largest
 * magnitude into [1, 2) (inv_scale[N] receives the inverse scales); the kernels scale every row of x the same way and undo
 * both on the float32 accumulators, so operands of ANY finite float32 magnitude are handled (fp16 alone overflows at 65504
 * and loses its lo half below 6e-5).                                                                                 */
SLK_API int slk_split_f16x2_f32(const float *w, int rows, int K, void *hi, void *lo, float *inv_scale, slk_stream_t stream);
SLK_API int slk_linear_rowstats_f16x3(const float *x, long ldx, const void *W_hi, const void *W_lo, const float *W_inv_scale,
                              const float *bias, float *y, long ldy, long M, int K, int N,
                              float *stats /* [M][2] or NULL */, slk_stream_t stream);
/* FeedForward.run (sloika/layers.py:157-158) on the same kernel: y = act(x.W^T + b); act one of linear / tanh / sigmoid /
 * relu / elu, otherwise SLK_ERR_UNSUPPORTED (use slk_gemm_bias_act_f32).  Both: K <= 192, N <= 2048.                  */
SLK_API int slk_gemm_bias_act_f16x3(const float *x, long ldx, const void *W_hi, const void *W_lo, const float *W_inv_scale,
                            const float *bias, float *y, long ldy, long M, int K, int N, int act, slk_stream_t stream);
/* The same product for rows longer than that kernel takes (csrc/gemm_bf16x6.hip: any K that is a multiple of 4; the dL/dx
 * products of the training step -- th.grad through T.dot in layers.py:157-158, :310-313, :1010-1021 -- whose K = 3n / 4n / nstate
 * exceeds 192): every float32 operand as three bf16 pieces, six bf16 MFMA terms per product in float32 accumulators (float32-grade,
 * float32's exponent range: gradients need no scaling).  W:[N][K] is cut once by slk_pack_bf16x3_f32 into
 * slk_pack_bf16x3_bytes(N, K) bytes.  act: linear / tanh / sigmoid; bias may be NULL.  SLK_ERR_UNSUPPORTED (->
 * slk_gemm_bias_act_f32) for other activations, K or ldx not multiples of 4, x or packed not 16-byte aligned. */
SLK_API size_t slk_pack_bf16x3_bytes(int N, int K);
SLK_API int slk_pack_bf16x3_f32(const float *W, int N, int K, void *packed, slk_stream_t stream);
SLK_API int slk_gemm_bias_act_bf16x6(const float *x, long ldx, const void *packed, const float *bias, float *y, long ldy, long M,
                             int K, int N, int act, slk_stream_t stream);
/* out = (x . W^T) * fun'(.), fun' in terms of the OUTPUT yref:[M][N] (rows ldyref apart) of the activation `dact` of the layer below
 * (tanh, sigmoid, relu, elu, linear): the dL/dx product of a layer and slk_act_backward_f32 of the layer below it in one pass.
 * Same shapes and packed weights as slk_gemm_bias_act_bf16x6; SLK_ERR_UNSUPPORTED likewise (-> the two calls). */
SLK_API int slk_gemm_dact_bf16x6(const float *x, long ldx, const void *packed, const float *yref, long ldyref, int dact, float *out,
                         long ldo, long M, int K, int N, slk_stream_t stream);
/* In-place row softmax of y:[M][N] (the second half of the above, exposed for testing).                     */
SLK_API int slk_softmax_rows_f32(float *y, long M, int N, slk_stream_t stream);
/* Row statistics only: stats[r] = (max_j logits[r][j], 1 / sum_j exp(logits[r][j] - max)); the posterior
 * exp(l - max) * inv_sum rebuilt from them is bit-identical to what slk_softmax_rows_f32 writes.  Lets the decoder
 * consume logits directly so the normalised posterior is never written (slk_viterbi_kmer_logits_f32).            */
SLK_API int slk_softmax_rowstats_f32(const float *logits, long M, int N, float *stats /* [M][2] */, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a4. Gru  (sloika/layers.py:952-1021; step :1010-1021; zero initial state :85-88; Reverse :1449-1450)
 *   slk_gru_recurrent_f32 consumes the time-parallel input projection
 *       vI[t][b][g*n + j] = x_t . iW[g*n+j] + b[g*n+j]   (g = 0 z, 1 r, 2 candidate; gate-block layout)
 *   computed by slk_gemm_bias_act_f32, and runs the sequential part
 *       z = gate(vI_z + h.sW_z^T)  r = gate(vI_r + h.sW_r^T)
 *       hbar = act(vI_c + (r*h).sW2^T)   h = z*h + (1-z)*hbar
 *   over t = 0..T-1 (reverse=0) or t = T-1..0 (reverse=1, implements Reverse(Gru) without copies).
 *   sW:[2n][n]  sW2:[n][n]  (reference shapes, [out][in]);  h_out element (t,b,j) at
 *   h_out[(t*B + b)*ldh + j]  (ldh >= n).
 *   vI is dense (rows 3n floats apart: the scan entries take no ldv) and must be 16-byte aligned: at n = 16, 32, ..., 144 the scan
 *   (gru_mfma_kernel of csrc/recurrent.hip) stages it into LDS with 16-byte LDS-DMA loads.  h_out may lie anywhere: with
 *   ldh % 4 == 0 and a 16-byte aligned h_out it is stored 16 bytes at a time, otherwise float by float (the same bits).
 *   lens (slk_gru_recurrent_ragged_f32): an entry outside [1, T] is clamped into it.
 * slk_gru_f32 = projection + recurrence; workspace >= slk_gru_workspace_bytes(T,B,n).
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_gru_recurrent_f32(const float *vI, const float *sW, const float *sW2, float *h_out, long ldh, int T, int B,
                          int n, int reverse, int act, int gate_act, slk_stream_t stream);
SLK_API size_t slk_gru_workspace_bytes(int T, int B, int n);
SLK_API int slk_gru_f32(const float *x, long ldx, const float *iW, const float *sW, const float *sW2, const float *bias,
                float *y, long ldy, int T, int B, int insize, int n, int reverse, int act, int gate_act,
                void *workspace, size_t workspace_bytes, slk_stream_t stream);
/* The whole layer with the RECURRENCE on the fp16 matrix pipe as well (csrc/gru_bar16.hip): every float32 operand of
 * h.sW^T and (r*h).sW2^T is split v = hi + lo into two fp16 halves and each product evaluated in float32 accumulators
 * (v_mfma_f32_16x16x32_f16) -- 22 significand bits per operand.  |h| <= 1 by construction; every row of x and of the
 * three weight matrices is scaled by a power of two to a maximum in [1, 2) before its split and the accumulators are
 * scaled back, so inputs and weights of any finite float32 magnitude are safe.  lens: NULL, or ragged lengths as
 * slk_gru_recurrent_ragged_f32; zr_out: NULL, or [T*B][2n] = [z | r] of every step (the training forward pass).
 * Execution plan: four waves per workgroup, one per SIMD with 512 registers each, stepping in lock step through two
 * s_barrier per time step; projection weights live in accumulation registers.  This is the plan sloika_amd.layers.Gru runs;
 * SLK_ERR_UNSUPPORTED for shapes without an instantiation ((insize, n) in {(96,96), (64,64), (32,96), (128,96), (64,96),
 * (48,32), (16,64)} -- BAR16_SHAPES of csrc/bar16_common.h is the source --, tanh / sigmoid).
 * A workgroup takes four chunks; a batch with more such workgroups than the device has CUs runs the eight-chunk plan of
 * csrc/gru_bar16d.hip instead (two four-chunk tiles through the same MFMAs), one with more eight-chunk workgroups than CUs
 * the sixteen-chunk plan of csrc/gru_bar16q.hip (four and eight chunks: bit-identical results; sixteen: to float32 rounding).
 * Bits 8-9 of `reverse` force a plan: 0 = by batch size, 1 / 2 / 3 = four / eight / sixteen chunks per workgroup.  Bit 10: the
 * four-chunk workgroups of a layer up to 64 wide may share a CU (no exclusive LDS request): for callers that run two such
 * launches side by side -- the directions of a birnn -- with more workgroups in all than the device has CUs.            */
SLK_API int slk_gru_bar16_f32(const float *x, long ldx, const float *iW, const float *sW, const float *sW2, const float *bias,
                      float *y, long ldy, int T, int B, int insize, int n, int reverse, int act, int gate_act,
                      const int32_t *lens, float *zr_out, slk_stream_t stream);
/* The four-chunk plan of slk_gru_bar16_f32 for weights that stay the same from call to call (inference), and for several layers at
 * once.  slk_gru_bar16_pack_f32 writes what every workgroup of that kernel otherwise makes in its prologue -- the fp16 hi / lo images
 * of sW, sW2 and iW in the order its lanes hold them, the rows' inverse scales and the bias (NULL: zeros) -- into `pack`
 * (slk_gru_bar16_pack_bytes(insize, n) bytes, 16-byte aligned; 0 bytes / SLK_ERR_UNSUPPORTED: no packed kernel for the shape; this
 * build has (96,96) and (64,64)).  The images are the bits the prologue makes; a pack is good until a weight changes.
 * slk_gru_bar16_stack_f32 runs nlayer (1 .. SLK_GRU_STACK_MAX) layers of one (insize, n) -- insize == n unless nlayer is 1 -- in ONE
 * launch of ceil(B / 4) workgroups: layer k reads layers[k].x (rows ldx floats apart, 16-byte aligned, ldx % 4 == 0) and writes
 * layers[k].h_out, which is usually layers[k+1].x.  A workgroup reads and writes the rows of its own four chunks only, so the
 * layers need no grid-wide step between them; every layer's result is, bit for bit, that of slk_gru_bar16_f32 with bits 8-9 of
 * `reverse` = 1 on the same operands.  `reverse` of a layer: bit 0 the direction, SLK_GRU_STACK_NO_LENS: the layer ignores `lens`
 * (scans and stores all T steps of every chunk, as slk_gru_bar16_f32 does with lens = NULL).  A layer's x and h_out must not
 * overlap; a layer may write where an earlier layer of the call READ (two buffers used in turn): a workgroup has consumed the
 * rows of its chunks by then and touches no others.  tanh / sigmoid only. */
#define SLK_GRU_STACK_MAX 8
#define SLK_GRU_STACK_NO_LENS 2
typedef struct {
    const float *x;
    long ldx;
    float *h_out;
    long ldh;
    const void *pack;
    int reverse;
    int reserved;
} slk_gru_stack_layer;
SLK_API size_t slk_gru_bar16_pack_bytes(int insize, int n);
SLK_API int slk_gru_bar16_pack_f32(const float *iW, const float *bias, const float *sW, const float *sW2, int insize, int n,
                           void *pack, slk_stream_t stream);
SLK_API int slk_gru_bar16_stack_f32(int nlayer, const slk_gru_stack_layer *layers, int insize, int n, int T, int B,
                            const int32_t *lens, slk_stream_t stream);
/* Host only: which instantiation a slk_gru_bar16_stack_f32 launch of batch B takes; `ragged` says whether any layer looks at lens
 * (lens != NULL and a layer without SLK_GRU_STACK_NO_LENS).  1: the full-batch kernel -- every workgroup has four chunks of T steps,
 * so its stores of h carry no predicate; taken when !ragged and B % 4 == 0.  0: the general kernel.  Same bits either way. */
SLK_API int slk_gru_bar16_stack_path(int B, int ragged);
/* Ragged batches (whole reads of different lengths, zero-padded to T steps; the reference calls reads one at a time,
 * sloika/basecall.py:88-121): lens[b] in [1, T] (int32, device) is the number of valid steps of chunk b.  Steps
 * t >= lens[b] of y / h_out are left untouched, and with reverse = 1 the scan of chunk b starts at ITS last step,
 * i.e. each chunk gets exactly what a call on the unpadded chunk alone would produce.                                */
SLK_API int slk_gru_recurrent_ragged_f32(const float *vI, const float *sW, const float *sW2, float *h_out, long ldh, int T, int B,
                                 int n, int reverse, int act, int gate_act, const int32_t *lens, slk_stream_t stream);
/* The same scan (Gru.step over a projection vI [T*B][ldv >= 3n] = x.iW^T + b in HBM; sloika/layers.py:1010-1021) for layers
 * too wide for the fused kernels: recurrent products on fp16 splits of weights and state, one wave per 16 neurons, four
 * chunks per workgroup stepping through two barriers per step (csrc/gru_scan1t.hip).  n = 112, 128 or 144
 * (models/pretrained.pkl, models/raw_1.00_rGr.py zero-padded), tanh / sigmoid, a projection of less than 4 GiB; anything
 * else SLK_ERR_UNSUPPORTED (-> slk_gru_recurrent_f32).  lens (int32 [B], device) or NULL as for
 * slk_gru_recurrent_ragged_f32.                                                                                          */
SLK_API int slk_gru_scan16_f32(const float *vI, long ldv, const float *sW, const float *sW2, float *y, long ldy, int T, int B, int n,
                       int reverse, int act, int gate_act, const int32_t *lens, slk_stream_t stream);
/* Force the portable (non-MFMA) recurrence kernel: 0 = auto, 1 = force generic.  Testing aid; passed per call
 * through the `_ex` form so that there is still no global state.                                            */
SLK_API int slk_gru_recurrent_f32_ex(const float *vI, const float *sW, const float *sW2, float *h_out, long ldh, int T,
                             int B, int n, int reverse, int act, int gate_act, int force_generic,
                             slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a6b. Lstm (sloika/layers.py:599-697; step :677-691 is authoritative: INTERLEAVED gate layout,
 *   row = j*4 + g with g = 0 update, 1 input gate, 2 forget gate, 3 output gate; peepholes p:[3][n]).
 *   vW[t][b][j*4+g] = x_t . iW[j*4+g] + b[j*4+g]  (from slk_gemm_bias_act_f32);  sW:[4n][n];
 *   p may be NULL (has_peep=False).  Output = the `out` half of the state (layers.py:697).
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_lstm_recurrent_f32(const float *vW, const float *sW, const float *p, float *out, long ldo, int T, int B,
                           int n, int reverse, int act, int gate_act, slk_stream_t stream);
SLK_API int slk_lstm_recurrent_ragged_f32(const float *vW, const float *sW, const float *p, float *out, long ldo, int T, int B,
                                  int n, int reverse, int act, int gate_act, const int32_t *lens /* see slk_gru_recurrent_ragged_f32 */,
                                  slk_stream_t stream);
/* The same scan with the recurrent product as a 3-term fp16 split on the barrier-stepped plan (csrc/lstm_scan16.hip; n a multiple
 * of 16 up to 128, tanh / sigmoid, vW 16-byte aligned and < 4 GiB; SLK_ERR_UNSUPPORTED otherwise -> slk_lstm_recurrent_f32).
 * lens may be NULL (all chunks T steps long). */
SLK_API int slk_lstm_scan16_f32(const float *vW, const float *sW, const float *p, float *out, long ldo, int T, int B, int n,
                        int reverse, int act, int gate_act, const int32_t *lens, slk_stream_t stream);
/* A whole Lstm layer of up to 64 units and up to 64 inputs in one kernel (csrc/lstm_fused16.hip): the scan of slk_lstm_scan16_f32 with
 * the projection vW = x.iW^T + b computed inside, four steps at a time, from x:[T][B][insize] (rows ldx floats apart) -- vW is never
 * written.  insize a multiple of 4 up to 64, n a multiple of 16 up to 64, tanh / sigmoid, x 16-byte aligned, ldx a multiple of 4;
 * SLK_ERR_UNSUPPORTED otherwise (-> projection GEMM + slk_lstm_scan16_f32).  bias, p and lens may be NULL. */
SLK_API int slk_lstm_fused16_f32(const float *x, long ldx, const float *iW, const float *sW, const float *bias, const float *p, float *y,
                         long ldy, int T, int B, int insize, int n, int reverse, int act, int gate_act, const int32_t *lens,
                         slk_stream_t stream);
SLK_API size_t slk_lstm_workspace_bytes(int T, int B, int n);
SLK_API int slk_lstm_f32(const float *x, long ldx, const float *iW, const float *sW, const float *bias, const float *p,
                 float *y, long ldy, int T, int B, int insize, int n, int reverse, int act, int gate_act,
                 void *workspace, size_t workspace_bytes, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a7 + a8. decode.prepare_post (sloika/decode.py:21-36) and decode.viterbi (sloika/decode.py:39-93),
 * batched over chunks (the reference decodes one [T,1,S] posterior per call, sloika/basecall.py:26-51).
 *   post : [T][B][nstate] float32, nstate = nbase^klen + 1, state 0 = blank/stay
 *   input_mode: SLK_POST_RAW   post is a network posterior: lp = log(min_prob + (1-min_prob)*post + 1e-10)
 *               SLK_POST_PLAIN lp = log(post + 1e-10)                        (decode.viterbi(log=False))
 *               SLK_POST_LOG   lp = post                                      (decode.viterbi(log=True))
 *   skip_pen  : decode.viterbi's skip_pen (float32 arithmetic as numpy does for float32 input)
 *   score_out : [B] best path score (float32)
 *   path_out  : [B][T] int32 k-mer states in time order, left aligned; entries >= len are -1
 *   len_out   : [B] path lengths (1 <= len <= T)
 * Tie-breaking is exactly the reference's: first maximum for step/skip/argmax (np.argmax), step vs skip tie
 * -> skip (decode.py:76), move vs stay tie -> stay (decode.py:81).  Integer outputs are bit-exact given the
 * same log-posteriors.  klen >= 3 (decode.py:50), nbase in {4,5} (any nbase with nbase^2 <= 64 works).
 * slk_log_post_f32 exposes the exact log-posterior transform the decoder applies (for tests).
 * ------------------------------------------------------------------------------------------------------- */
#define SLK_POST_RAW 0
#define SLK_POST_PLAIN 1
#define SLK_POST_LOG 2
#define SLK_POST_LN 3 /* slk_log_post_f32 only: lp = log(post), no eta (np.log(trans), sloika/transducer.py:30) */
SLK_API size_t slk_viterbi_kmer_workspace_bytes(int T, int B, int nbase, int klen);
/* What slk_viterbi_kmer_*_f32 will launch for a shape (host only: nothing is launched, no device is needed).  The decoder takes
 * its own decisions from the same function, so this is what runs; tests compute their edge lengths from it.
 *   ws_align : alignment of the workspace in bytes, a power of two (16 or more: fully aligned)
 *   kernel       : which forward kernel (below)
 *   blank_steps  : steps per block of blank-column log-posteriors the forward kernel evaluates at once (0: every step on its own)
 *   staged_rows  : traceback rows the forward kernel collects in LDS before it stores them (0: every row is stored at once)
 *   tb_row_bytes : bytes of one traceback row of one chunk
 *   walker_rows  : traceback rows per block the backtrace stages in LDS (min(12288 / tb_row_bytes, T))
 *   walker_dma   : 1 if the backtrace stages through its LDS-DMA ring of three blocks, 0 for the plain copy loop           */
#define SLK_VIT_KERNEL_GENERIC 0    /* any nbase: one workgroup per chunk, a traceback byte per state */
#define SLK_VIT_KERNEL_WORKGROUP4 1 /* nbase 4: one workgroup per chunk, packed traceback */
#define SLK_VIT_KERNEL_WAVE4 2      /* nbase 4, large batches: one wave per chunk, packed traceback */
typedef struct slk_viterbi_plan {
    int kernel, blank_steps, staged_rows, tb_row_bytes, walker_rows, walker_dma;
} slk_viterbi_plan;
SLK_API int slk_viterbi_kmer_plan(int T, int B, int nbase, int klen, int ws_align, slk_viterbi_plan *plan);
SLK_API int slk_viterbi_kmer_f32(const float *post, int T, int B, int nbase, int klen, float skip_pen, int input_mode,
                         float min_prob, void *workspace, size_t workspace_bytes, float *score_out,
                         int32_t *path_out, int32_t *len_out, slk_stream_t stream);
SLK_API int slk_log_post_f32(const float *post, float *lpost, size_t count, int input_mode, float min_prob,
                     slk_stream_t stream);
/* Softmax.run + decode_post in one pass over the LOGITS (sloika/layers.py:309-314 + sloika/basecall.py:26-51):
 * logits: rows (t,b) of nstate floats, `ld` floats apart, = x.W^T + b;  stats:[T*B][2] from slk_linear_rowstats_f32
 * (or slk_softmax_rowstats_f32 for dense logits).  Same outputs as
 * slk_viterbi_kmer_f32(SLK_POST_RAW) on the normalised posterior, bit for bit.  slk_log_post_logits_f32 exposes the
 * log-posterior it decodes (for tests).                                                                          */
SLK_API int slk_viterbi_kmer_logits_f32(const float *logits, long ld /* floats between rows, >= nstate */, const float *stats,
                                int T, int B, int nbase, int klen, float skip_pen, float min_prob, void *workspace,
                                size_t workspace_bytes, float *score_out, int32_t *path_out, int32_t *len_out,
                                slk_stream_t stream);
/* Ragged form (see slk_gru_recurrent_ragged_f32): chunk b is decoded over its first lens[b] steps only; path_out rows keep
 * the padded length T.                                                                                               */
SLK_API int slk_viterbi_kmer_logits_ragged_f32(const float *logits, long ld, const float *stats, int T, int B, int nbase, int klen,
                                       float skip_pen, float min_prob, const int32_t *lens, void *workspace,
                                       size_t workspace_bytes, float *score_out, int32_t *path_out, int32_t *len_out,
                                       slk_stream_t stream);
SLK_API int slk_log_post_logits_f32(const float *logits, long ld, const float *stats, float *lpost /* dense [rows][nstate] */,
                            size_t rows, int nstate, float min_prob, slk_stream_t stream);
/* The same chain from the Softmax layer's INPUT: x.W^T + b, softmax, prepare_post, log and the Viterbi forward pass in one
 * kernel, so that the [T][B][nstate] logits never exist in memory (sloika/layers.py:309-314 -> sloika/decode.py:21-36 ->
 * :39-93; what basecall.decode_post(calc_post(x)) computes from the last hidden layer on, sloika/basecall.py:26-51, 119).
 *   x    : rows (t, b) of K floats, ldx floats apart (ldx % 4 == 0, 16-byte aligned), row index t*B + b
 *   pack : the layer's weights W[nstate][K], b[nstate] (or NULL) re-laid-out once by slk_softmax_viterbi_pack_f32 into a
 *          buffer of slk_softmax_viterbi_pack_bytes(K, nbase, klen) bytes (fp16 hi/lo MFMA fragments, column scales)
 *   lens : per-chunk step counts for a ragged batch, or NULL
 *   plan : chunks per workgroup: 0 (the build's default) or 2; 4 (two score chains per lane, half as many workgroups) is
 *          compiled only with -DSV_WITH_NCH4 (measured no faster) and returns SLK_ERR_UNSUPPORTED otherwise; results do
 *          not depend on it
 *   lp_dump : NULL, or [T][B][nstate] floats that receive the log-posteriors the dynamic programme consumed (tests decode
 *          THESE with the oracle: paths and scores are bit-exact functions of them)
 *   workspace: slk_softmax_viterbi_workspace_bytes(T, B, nbase, klen) bytes, 16-byte aligned (one traceback byte per four
 *          k-mers and step: a quarter of slk_viterbi_kmer_workspace_bytes, which is also accepted)
 * Products are 3-term fp16 splits with float32 accumulation like slk_linear_rowstats_f16x3.  This build has the kernel for
 * nbase 4, klen 5 and K in {64, 96, 112, 128}; anything else returns SLK_ERR_UNSUPPORTED (pack_bytes returns 0) and the
 * caller uses slk_linear_rowstats_* + slk_viterbi_kmer_logits_f32.                                                        */
SLK_API size_t slk_softmax_viterbi_pack_bytes(int K, int nbase, int klen);
SLK_API size_t slk_softmax_viterbi_workspace_bytes(int T, int B, int nbase, int klen);   /* 0: shape outside the fused kernel */
SLK_API int slk_softmax_viterbi_pack_f32(const float *W, const float *bias, int K, int nbase, int klen, void *pack,
                                 slk_stream_t stream);
SLK_API int slk_softmax_viterbi_f32(const float *x, long ldx, const void *pack, int K, int T, int B, int nbase, int klen,
                            float skip_pen, float min_prob, const int32_t *lens, int plan, void *workspace,
                            size_t workspace_bytes, float *score_out, int32_t *path_out, int32_t *len_out, float *lp_dump,
                            slk_stream_t stream);
/* f8. The sum-product twin of slk_viterbi_kmer_f32 (design/lattice_marginals.md): over the SAME lattice -- per row a stay
 * (weight p[i][0]), a step (p[i][1+s]) or a skip (exp(-skip_pen) p[i][1+s]) into k-mer state s, row 0 weighing p[0][1+s]; p the
 * float32 values slk_prepare_post_f32 gives (SLK_POST_RAW; the input itself for SLK_POST_PLAIN) widened to float64; the 1e-10 of
 * decode.viterbi's log is no part of the weights -- the sum Z of all path weights, the share gamma[i][s] of Z that passes through
 * s at row i, and for every position of the called path a confidence.
 *   post       : [T][B][N + 1] float32 in the network layout, N = nbase^klen; input_mode SLK_POST_RAW or SLK_POST_PLAIN
 *                (SLK_POST_LOG / SLK_POST_LN: SLK_ERR_UNSUPPORTED -- the sum needs the weights, not their logarithms)
 *   klen >= 3, nbase 4 or 5, N <= 1024; anything else: SLK_ERR_UNSUPPORTED (workspace_bytes: 0), nothing is written
 *   lens       : NULL, or [B] int32 on the device: chunk b owns its first lens[b] rows, clamped to 1 .. T
 *   score_out, path_out, len_out : what slk_viterbi_kmer_f32 returns for the chunk's rows, bit for bit (the same float32
 *                recursion and tie rules)
 *   move_row   : [B][T] int32, move_row[b][j] = the row at which the path enters its j-th state (move_row[b][0] = 0); position j
 *                dwells on rows move_row[j] .. move_row[j + 1] - 1, the last one up to the chunk's last row
 *   conf       : [B][T] float64, conf[b][j] = the largest gamma[i][path[j]] over the rows i of position j's dwell
 *   logz       : [B] float64, log Z (natural)
 *   gamma      : NULL, or [T][B][N] float32: each float64 value rounded once; rows behind a chunk's own are 0
 *   entries of move_row / conf at or behind len_out[b] are -1 / 0.
 * The sum runs in float64, rows scaled by exact powers of two.  A chunk's outputs have the same bits alone, in any batch, with or
 * without gamma.  workspace: 8-byte aligned, slk_viterbi_marginals_workspace_bytes(T, B, nbase, klen) bytes (9 N + 20 per row and
 * chunk: the float64 forward rows and a traceback byte per state), else SLK_ERR_WORKSPACE and nothing is written; T, B < 1, a null
 * pointer, min_prob outside [0, 1): SLK_ERR_INVALID_ARG. */
SLK_API size_t slk_viterbi_marginals_workspace_bytes(int T, int B, int nbase, int klen);   /* host only; 0 for a refused shape */
SLK_API int slk_viterbi_marginals_f32(const float *post, int T, int B, int nbase, int klen, float skip_pen, int input_mode,
                              float min_prob, const int32_t *lens, void *workspace, size_t workspace_bytes, float *score_out,
                              int32_t *path_out, int32_t *len_out, int32_t *move_row, double *conf, double *logz, float *gamma,
                              slk_stream_t stream);
/* f8. slk_viterbi_marginals_f32 with checkpointed forward rows (design/lattice_marginals.md 8): the same arguments, limits and
 * refusals, and on the same input the same bits in every output, for every legal `every`.  Pass 1 keeps the forward state of every
 * `every`-th row only (row 0 included); pass 2 recomputes each segment of `every` rows into LDS just before it walks down it, so no
 * forward row travels to device memory and the workspace shrinks about `every`-fold.
 *   every      : rows per checkpoint, K.  0: the launcher's choice for N (36 KiB of LDS for the segment: 4 at N = 1024, more for a
 *                smaller N, at most 64); < 0: SLK_ERR_INVALID_ARG; a K whose segment buffer of 9 N K bytes does not fit into the
 *                160 KiB of a CU's LDS beside the kernel's 21.1 KiB (K >= 16 at N = 1024): SLK_ERR_UNSUPPORTED; nothing is written
 *   workspace  : 8-byte aligned, slk_viterbi_marginals_ckpt_workspace_bytes(T, B, nbase, klen, every) bytes: ceil(T / K)
 *                checkpoints of 13 N bytes per chunk (float64 forward row, float32 max-plus row, a traceback byte per state) and 20
 *                bytes per row and chunk, else SLK_ERR_WORKSPACE and nothing is written. */
SLK_API size_t slk_viterbi_marginals_ckpt_workspace_bytes(int T, int B, int nbase, int klen, int every); /* host only; 0 when refused */
SLK_API int slk_viterbi_marginals_ckpt_f32(const float *post, int T, int B, int nbase, int klen, float skip_pen, int input_mode,
                                   float min_prob, const int32_t *lens, int every, void *workspace, size_t workspace_bytes,
                                   float *score_out, int32_t *path_out, int32_t *len_out, int32_t *move_row, double *conf,
                                   double *logz, float *gamma, slk_stream_t stream);
/* decode.prepare_post on its own: out = min_prob + (1-min_prob)*post (decode.py:36).                        */
SLK_API int slk_prepare_post_f32(const float *post, float *out, size_t count, float min_prob, slk_stream_t stream);
/* decode.argmax (decode.py:5-18), batched: per (b) the states with argmax != blank, minus 1 if
 * zero_is_blank; same output convention as slk_viterbi_kmer_f32.                                            */
SLK_API int slk_argmax_decode_f32(const float *post, int T, int B, int nstate, int zero_is_blank, int32_t *path_out,
                          int32_t *len_out, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a10. The decoder of NON-transducer models: what basecall.decode_post(transducer=False) runs (sloika/basecall.py:44, 47-50),
 * batched over reads: decode.prepare_post(drop_bad=True) (sloika/decode.py:31-36), olddecode.estimate_transitions
 * (sloika/olddecode.py:93-117), olddecode.decode_profile (:13-73) and, without weights, olddecode.decode_simple (:85-90).
 * olddecode.decode_transition (:76-82) raises in the reference and has no entry point.
 *   nbase 4 only (basecall.py:48), 3 <= klen <= 6; anything else: SLK_ERR_INVALID_ARG (workspace_bytes: 0).  N = 4^klen.
 *   lens : NULL, or [B] int32 rows per read (0 <= lens[b] <= T) -- a ragged batch; read b then gets what a call on its first
 *          lens[b] rows alone gives.  One workgroup per read: a read's bits do not depend on what shares the launch.
 * slk_prepare_post_drop_bad_f32: post [T][B][N + 1] -> out [T][B][N]: of read b the rows whose FIRST maximum is not column 0,
 *   left aligned, without column 0, divided by their float32 sum (taken in numpy's summation order) and floored with min_prob:
 *   bit for bit what numpy writes.  kept[b] = rows written (rows behind them are not touched); kept_rows: NULL or [B][T], the
 *   indices of the rows kept, -1 padded.  kept is the `lens` of the two calls below.
 * slk_estimate_transitions_f64: post [T][B][N] float32, 16-byte aligned -> trans_out [B][T][3] float64 (stay, step, skip; rows
 *   sum to 1; rows >= lens[b] are 0), sums in float64 where the reference sums in float32.  have_trans = 0: the prior is the read's own
 *   normalised column sums (trans=None), else (t_stay, t_step, t_skip).  log_trans_out: NULL or [B][T][3], log(eta + trans) of the
 *   same pass (basecall.py:50).
 * slk_decode_profile_f64: post [T][B][N] float32, 16-byte aligned; input_mode SLK_POST_PLAIN (lp = log(post + 1e-10) in float32) or
 *   SLK_POST_LOG; trans: NULL (decode_simple: no weights and then no log 4 / log 16 either, olddecode.py:27-32) or [B][T][3]
 *   float64 LOG weights, row t - 1 used by step t; log_slip = log(1e-10 + slip).  The recurrence runs in float64 as numpy's does;
 *   ties as the reference resolves them: of stay, slip, step, skip the last that reaches the maximum (np.where(score > new, ...)),
 *   first maximum among the 4 step / 16 skip predecessors and for the slip source and the final state (np.argmax).  Path and
 *   score are bit-exact functions of the log-posteriors and the weights.
 *   score_out [B] float64 (NaN for an empty read); path_out [B][T] int32, one state per row, -1 padded; len_out [B] = lens.
 *   workspace >= slk_decode_profile_workspace_bytes(T, B, nbase, klen), 16-byte aligned (a traceback byte per state and step).
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_prepare_post_drop_bad_f32(const float *post, int T, int B, int nbase, int klen, float min_prob, const int32_t *lens,
                                  float *out, int32_t *kept, int32_t *kept_rows, slk_stream_t stream);
SLK_API int slk_estimate_transitions_f64(const float *post, int T, int B, int nbase, int klen, int have_trans, double t_stay,
                                 double t_step, double t_skip, double eta, const int32_t *lens, double *trans_out,
                                 double *log_trans_out, slk_stream_t stream);
SLK_API size_t slk_decode_profile_workspace_bytes(int T, int B, int nbase, int klen);
SLK_API int slk_decode_profile_f64(const float *post, int T, int B, int nbase, int klen, int input_mode, const double *trans,
                           double log_slip, const int32_t *lens, void *workspace, size_t workspace_bytes, double *score_out,
                           int32_t *path_out, int32_t *len_out, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * f1. States -> bases (sloika/bio.py:160-179 max_overlap, :206-225 reduce_kmers, :228-237 kmers_to_sequence; what
 *   basecall.SeqPrinter.write does with a call, basecall.py:157-163), for a whole batch of decoded paths on the device.
 *   A state is the base-`nbase` number of its k-mer (first letter most significant, bio.py:12-24), so the overlap test
 *   k1[i:] == k2[:-i] is  s1 mod nbase^(k-i) == s2 div nbase^i; the smallest such i is the move (k if none, 0 for a
 *   repeated state unless always_move).  paths:[B][ld] int32, lens:[B]; alphabet: the letters packed little-endian in 8
 *   bytes; out:[B][cap] bytes with cap >= klen * max(lens); nbases[b] = letters written for read b.
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_paths_to_bases(const int32_t *paths, long ld, const int32_t *lens, int B, int klen, int nbase, int always_move,
                       unsigned long long alphabet, uint8_t *out, long cap, int32_t *nbases, slk_stream_t stream);
/* f8. The same letters, byte for byte, and a Phred value beside each: qual:[B][cap] bytes, qual[b][m] = the value of the path
 *   position that emitted letter m (the first position emits klen letters, a later one its move's).  conf:[B][ldc] float64, one
 *   confidence per path position (slk_viterbi_marginals_f32); thresholds:[qmax] float64 ON THE DEVICE, thresholds[k - 1] =
 *   10^(-k/10) as the host's float64 pow gives it, 1 <= qmax <= 93.  The value is the number of k in 1 .. qmax with
 *   1.0 - conf <= thresholds[k - 1]: comparisons only, no log on the device, an exact integer that a search of the same table
 *   reproduces (a conf that is NaN gives 0). */
SLK_API int slk_paths_to_bases_qual(const int32_t *paths, long ld, const int32_t *lens, const double *conf, long ldc,
                            const double *thresholds, int qmax, int B, int klen, int nbase, int always_move,
                            unsigned long long alphabet, uint8_t *out, uint8_t *qual, long cap, int32_t *nbases,
                            slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a9. The reference's only true FFI: viterbi_helpers.slip_update (sloika/viterbi_helpers.pyx:12-35), and
 * its caller transducer.map_to_sequence (sloika/transducer.py:14-73).
 *   slk_slip_update_f32: x:[n] -> from_score:[n] float32, from_pos:[n] int64; n >= 3.
 *   slk_map_to_sequence_f32: ltrans:[nev][nst] LOG-space float32, seq:[npos] int32 state indices,
 *     prior_initial / prior_final: [npos] float64 or NULL (the reference adds float64 priors into the
 *     float32 score vector, transducer.py:39-41,63-64); score_out:[1]; path_out:[nev] int32.
 *     workspace >= slk_map_to_sequence_workspace_bytes(nev, npos).  npos >= 3.
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_slip_update_f32(const float *x, int n, float slip, float *from_score, int64_t *from_pos,
                        slk_stream_t stream);
SLK_API size_t slk_map_to_sequence_workspace_bytes(int nev, int npos);
SLK_API int slk_map_to_sequence_f32(const float *ltrans, int nev, int nst, const int32_t *seq, int npos, float slip,
                            const double *prior_initial, const double *prior_final, void *workspace,
                            size_t workspace_bytes, float *score_out, int32_t *path_out, slk_stream_t stream);
/* Batched form of the same call (the reference remaps reads one by one: bin/chunkify.py `remap` ->
 * transducer.map_to_sequence, sloika/transducer.py:14-73): `nread` reads of different lengths, concatenated.
 *   ev_off:[nread+1] int64 -- read b owns rows ev_off[b]..ev_off[b+1] of ltrans ([sum nev][nst]) and of path_out;
 *   pos_off:[nread+1] int64 -- ... and positions pos_off[b]..pos_off[b+1] of seq / prior_initial / prior_final;
 *   ws_off:[nread] int64 -- offset (in int32 elements) of read b's nev_b*npos_b traceback inside `workspace`;
 *   max_npos = the longest sequence (sizes the LDS request: 28 bytes per position of the 160 KB, npos <= 5846); score_out:[nread].
 * A read with fewer than 3 positions or no events gets score -inf and its path is left untouched. */
SLK_API int slk_map_to_sequence_batch_f32(const float *ltrans, int nst, const int64_t *ev_off, const int32_t *seq,
                                  const int64_t *pos_off, int nread, int max_npos, float slip,
                                  const double *prior_initial, const double *prior_final, void *workspace,
                                  const int64_t *ws_off, float *score_out, int32_t *path_out, slk_stream_t stream);

/* The same remap for references of any length (design/remap_long.md): the two entries above keep their whole state in LDS and
 * refuse more than 5846 positions; these keep the two score rows in the workspace, behind the traceback, and one tile of positions
 * in LDS at a time.  Score and path are bit for bit those of the entries above (and of the reference).
 *   tile: positions per tile, a multiple of 64 from 64 to 6784 (what 160 KB of LDS hold); 0 selects the default, 4096.  Another
 *     value: SLK_ERR_INVALID_ARG.
 *   slk_map_to_sequence_long_workspace_bytes(nev, npos, tile): the nev * npos int32 traceback plus two float32 score rows of
 *     npos + 16 each; 0 for a bad argument.  Host only.
 *   slk_map_to_sequence_long_f32: the arguments of slk_map_to_sequence_f32 and `tile`; a workspace smaller than the function above
 *     gives SLK_ERR_WORKSPACE.
 *   slk_map_to_sequence_long_batch_f32: the arguments of slk_map_to_sequence_batch_f32 and `tile`; ws_off[b] is the offset (in int32
 *     elements) of read b's workspace, slk_map_to_sequence_long_workspace_bytes(nev_b, npos_b, tile) / 4 elements long; as in that
 *     entry the length of `workspace` is the caller's to get right.  max_npos bounds the tile (short reads ask for little LDS) and
 *     has no upper limit.  A read with fewer than 3 positions or no events gets score -inf; its path and its workspace are left
 *     untouched.
 * Nothing is written when a call is refused. */
SLK_API size_t slk_map_to_sequence_long_workspace_bytes(int nev, int npos, int tile);
SLK_API int slk_map_to_sequence_long_f32(const float *ltrans, int nev, int nst, const int32_t *seq, int npos, float slip,
                                 const double *prior_initial, const double *prior_final, void *workspace,
                                 size_t workspace_bytes, int tile, float *score_out, int32_t *path_out, slk_stream_t stream);
SLK_API int slk_map_to_sequence_long_batch_f32(const float *ltrans, int nst, const int64_t *ev_off, const int32_t *seq,
                                       const int64_t *pos_off, int nread, int max_npos, float slip,
                                       const double *prior_initial, const double *prior_final, void *workspace,
                                       const int64_t *ws_off, int tile, float *score_out, int32_t *path_out,
                                       slk_stream_t stream);

/* f3, second half: the labels of raw_chunkify (sloika/tools/chunkify_raw.py:164-210), from the mapping table raw_remap
 * (chunkify_raw.py:260-296) produces.  Integer work, bit-exact.  `alphabet` is a HOST string of `nbase` <= 8 letters
 * (batch.init_chunk_identity_worker's alphabet, sloika/batch.py:17-27); every other pointer is device memory.
 * `status` (device int, zeroed by the caller) gets bit 0 set for a letter outside the alphabet and bit 1 for a reference
 * position outside the reference string -- the cases in which the reference's `batch.kmer_to_state[...]` raises KeyError.
 *
 * slk_kmer_labels_i32 = labels_from_mapping_table (chunkify_raw.py:117-136): kmers:[n][old_klen] bytes (the table's 'kmer'
 *   column), labels_out[i] = state of the middle `klen` letters + index_from, or -1 for a foreign letter. */
SLK_API int slk_kmer_labels_i32(const uint8_t *kmers, int64_t n, int old_klen, int klen, const char *alphabet, int nbase,
                                int index_from, int32_t *labels_out, int *status, slk_stream_t stream);
/* slk_raw_chunk_labels_i32 = the non-interpolated branch (chunkify_raw.py:194-204) for `nread` reads in one launch (the
 * reference runs one read per worker call, chunkify_raw.py:299-337).  The tables are the TRIMMED ones (after
 * trim_signal_and_mapping(signal, table, 0, nchunk*chunk_len), chunkify_raw.py:174), concatenated:
 *   start, move:[sum nevent] int64 columns; event_label:[sum nevent] = slk_kmer_labels_i32 of the 'kmer' column;
 *   ev_off:[nread+1]; nchunk:[nread] chunks of read b; lab_off:[nread] offset (in elements) of read b's
 *   [nchunk_b][ceil(chunk_len / downsample)] int32 labels inside labels_out; max_nchunk = max(nchunk).
 * workspace: slk_raw_chunk_labels_workspace_bytes(sum nevent) bytes. */
SLK_API size_t slk_raw_chunk_labels_workspace_bytes(int64_t nevent);
SLK_API int slk_raw_chunk_labels_i32(const int64_t *start, const int64_t *move, const int32_t *event_label,
                                     const int64_t *ev_off, int nread, const int64_t *nchunk, const int64_t *lab_off,
                                     int64_t max_nchunk, int chunk_len, int downsample, void *workspace,
                                     size_t workspace_bytes, int32_t *labels_out, slk_stream_t stream);
/* slk_raw_chunk_labels_interp_i32 = the interpolated branch (chunkify_raw.py:187-193 with interpolate_pos /
 * interpolate_labels :86-114) for one read: label o belongs to sample o * downsample; position = np.interp over the block
 * mid-times in float64, evaluated like numpy's C loop, then np.around(. - 0.5 * klen + 1e-10).
 *   forward != 0: direction '+', ref_anchor = ref_start;  forward == 0: direction '-', ref_anchor = ref_stop.
 *   map_klen = length of the table's k-mers; reference:[ref_len] bytes; pos_out (optional):[nlabel] int64 positions.
 *   times (optional):[nlabel] float64 -- the caller's own times (the closures interpolate_pos / interpolate_labels return
 *   take any), instead of o * downsample;  zero_repeats != 0 applies line :191 (raw_chunkify), 0 leaves every label.
 * labels_out[o] = state + 1 of reference[pos:pos+klen], 0 where pos repeats the previous label's, -1 on a status error;
 * labels_out may be NULL when only positions are wanted (then reference / alphabet are not read). */
SLK_API int slk_raw_chunk_labels_interp_i32(const int64_t *start, const int64_t *length, const int64_t *seq_pos,
                                            int64_t nevent, int map_klen, int forward, int64_t ref_anchor,
                                            const uint8_t *reference, int64_t ref_len, int klen, const char *alphabet,
                                            int nbase, int64_t nlabel, int downsample, const double *times,
                                            int zero_repeats, int32_t *labels_out, int64_t *pos_out, int *status,
                                            slk_stream_t stream);

/* f3 for event models: `chunkify remap` (sloika/batch.py:143-190, sloika/tools/chunkify_with_remap.py:52-59) for a ragged set of
 * reads (csrc/event_remap.hip).
 *
 * slk_remap_pack_log_post_f32 = log(prepare_post(post)) (batch.py:146 with decode.py:36, then transducer.py:30 np.log(trans)) of
 *   the reads of a ragged batch, packed for slk_map_to_sequence_batch_f32:
 *   post: the network-layout posterior, row (t, b) of S floats at post + t * row_stride + b * batch_stride (strides in floats,
 *   batch_stride >= S; the tensor need not be dense); nstep:[B] int32 steps of read b; ev_off:[B+1] int64; out:[ev_off[B]][S].
 *   out row ev_off[b] + t = what slk_prepare_post_f32 followed by slk_log_post_f32(SLK_POST_LN) gives for row t of read b, bit
 *   for bit (the same device functions).  Rows t >= min(nstep[b], ev_off[b+1] - ev_off[b], T) are neither read nor written. */
SLK_API int slk_remap_pack_log_post_f32(const float *post, long row_stride, long batch_stride, int T, int B, int S,
                                        const int32_t *nstep, const int64_t *ev_off, float min_prob, float *out,
                                        slk_stream_t stream);
/* slk_event_remap_labels_i32 = the labels of batch.chunkify (batch.py:69-78) on the table batch.remap returns (batch.py:157-158:
 *   seq_pos = path, kmer = kmers[path], so model_kmer_len == kmer_len and the label is the k-mer's state + 1), and the strand-list
 *   fields of tools/chunkify_with_remap.py:57-58, for `nread` reads straight from the DP's paths:
 *   path:[sum nev] int32 and ev_off:[nread+1] as slk_map_to_sequence_batch_f32 leaves them; seq:[sum npos] int32 (state + 1 per
 *   reference position) with pos_off:[nread+1]; row_off:[nread] int64 -- read b's (nev_b / chunk_len) * chunk_len labels start at
 *   labels_out[row_off[b]]; labels_out:[total_rows].
 *   label of event e = seq[path[e]], 0 where e % chunk_len != 0 and path[e] == path[e-1] (a chunk's first event keeps its label).
 *   stats_out:[nread][3] int32 over ALL events of a read: #{e >= 1: path[e] == path[e-1]} (np.sum(np.ediff1d(path, to_begin=1)
 *   == 0)), min(path), max(path).
 *   status (device int, zeroed by the caller): bit 1 for a path entry outside [0, npos_b) (label -1; nothing is read through
 *   it), bit 2 for a read whose labels would not fit into total_rows (none of them is written). */
SLK_API int slk_event_remap_labels_i32(const int32_t *path, const int64_t *ev_off, const int32_t *seq, const int64_t *pos_off,
                                       int nread, int chunk_len, const int64_t *row_off, int64_t total_rows, int32_t *labels_out,
                                       int32_t *stats_out, int *status, slk_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * f2. The training step: bin/train_network.py:124-142 (`wrap_network`: loss, accuracy, th.grad, updates.adam) and
 * sloika/updates.py:9-103.  The reference crosses into Theano once per batch (`fg(indata, labels, weights, rate)`,
 * train_network.py:308); its gradient comes from automatic differentiation, here the reverse pass of Convolution
 * (layers.py:417-419), Gru.step (layers.py:1010-1021) and Softmax (layers.py:309-314) is explicit (csrc/train.hip).
 * Rows are m = t*B + b throughout.
 *
 * Gate recompute (forward values the reverse scan needs, recomputed time-parallel from the finished forward pass):
 *   slk_train_pack_xh_f32:  xh[m] = [x[m] (I) | h_prev[m] (N)], h_prev = h at the previous scan step, 0 at the scan start
 *   slk_train_pack_xrh_f32: xrh[m] = [x[m] | r[m] * h_prev[m]] with zr[m] = [z | r] ([M][2N]) (kept for callers that
 *     want the candidate as a GEMM too: c = tanh(xrh . [iW[2n:] | sW2]^T + b[2n:]))
 *   then zr = sigmoid(xh . [iW[:2n] | sW]^T + b[:2n]) is a plain slk_gemm_bias_act_f16x3 / slk_gemm_bias_act_f32 call.
 * slk_gru_backward_f32: the reverse scan.  dy:[T][B] rows lddy apart = dL/dh from the layer above; hprev: h at the
 *   previous scan step per row (rows ldhp apart: the h half of the packed xh rows, or a view of the layer output shifted
 *   by one step over a zero row); zr:[M][2n] the activated gates (recomputed as above, or saved by
 *   slk_gru_bar16_f32 with zr_out); h: the layer's own forward output (rows ldh apart), from which the candidate of every step is recovered as (h_t - z h_prev) / (1 - z);
 *   writes da:[M][3n] = dL/dvI = [daz | dar | dac] and rh:[M][n] = r * h_prev.  n in {16,32,48,64,96,112,128,144},
 *   tanh / sigmoid, else SLK_ERR_UNSUPPORTED.
 *   Weight gradients follow as contractions over m (slk_gemm_tn_f32): diW = da^T x, dsW = da[:, :2n]^T h_prev,
 *   dsW2 = da[:, 2n:]^T rh, db = da^T 1 (its colsum output); and dL/dx = da . iW (slk_gemm_bias_act_f32 with iW^T).
 * slk_softmax_xent_grad_f32: loss terms and dL/dlogits of train_network.py:128-136, in place over the logits written by
 *   slk_linear_rowstats_* (stats:[M][2] = max, 1/sum).  loss_rows[m] and correct_rows[m] are already divided by the
 *   number of counted positions (T - 2 drop) * B, so their sums are the data term of the loss and the accuracy.
 *   Columns nstate..ld-1 of every row are set to zero.  labels must lie in [0, nstate).  At min_prob == 0 a label whose posterior
 *   underflows in float32 gives that row an infinite loss and a non-finite gradient, as the reference does (the other rows are not
 *   affected); train_network.py's own default is above 0.
 * slk_reduce_sum_f32: out[0] = sum x (square = 0) or sum x^2 (square = 1: updates.param_sqr), float64, fixed order.
 * slk_gemm_tn_f32: C[N1][N2] (rows ldc apart) = A^T B, A:[M][N1] rows lda apart, B:[M][N2] rows ldb apart; when colsum is
 *   given it also receives the column sums of A (A^T 1: the bias gradient) from the same pass.
 * slk_act_backward_f32: out = dy * fun'(pre-activation) written through the OUTPUT y; linear/tanh/sigmoid/relu/elu.
 * slk_train_im2col_cin1_f32: window rows of a one-feature Convolution, cols:[Tout*B][winlen] (dW = dpre^T cols).
 * slk_adamski_update_f32: updates.py:77-87 over flat buffers with this step's lr_t / momentum_decay (updates.py:73-76);
 *   g = clip(grad * gscale + 2 l2 param).   slk_sgd_update_f32: updates.py:9-33.
 * ------------------------------------------------------------------------------------------------------- */
SLK_API int slk_train_pack_xh_f32(const float *x, long ldx, const float *h, long ldh, float *xh, int T, int B, int insize, int n,
                          int reverse, slk_stream_t stream);
SLK_API int slk_train_pack_xrh_f32(const float *xh, const float *zr, float *xrh, long M, int insize, int n, slk_stream_t stream);
SLK_API int slk_gru_backward_f32(const float *dy, long lddy, const float *hprev, long ldhp, const float *zr, const float *h, long ldh,
                         const float *sW, const float *sW2, float *da, float *rh, int T, int B, int n, int reverse,
                         int act, int gate_act, slk_stream_t stream);
/* The same reverse scan with its two products as fp16 splits on the barrier-stepped plan of the forward kernels (csrc/gru_bwd16.hip:
 * one wave per 16 units, two MFMAs per product, operand images scaled per chunk and step by a power of two from a bound -- gradients
 * have no natural range).  Same arguments; n a multiple of 16 up to 128, tanh / sigmoid, fewer than 4 GiB per operand;
 * SLK_ERR_UNSUPPORTED otherwise (-> slk_gru_backward_f32).  Results agree with it to float32 rounding of the products. */
SLK_API int slk_gru_backward16_f32(const float *dy, long lddy, const float *hprev, long ldhp, const float *zr, const float *h, long ldh,
                         const float *sW, const float *sW2, float *da, float *rh, int T, int B, int n, int reverse,
                         int act, int gate_act, slk_stream_t stream);
/* ... and with the layer's dL/dx = da . iW (updates.py:67: th.grad through the projection of layers.py:1011, iW:[3n][insize]) formed in
 * the same pass from the operand images of each step (they ARE da of that step as fp16 pairs): dx:[T][B] rows of insize floats, lddx
 * apart, float32-grade like the pass's own products.  n a multiple of 16 up to 96, insize <= 64 (n <= 64) or 96; SLK_ERR_UNSUPPORTED
 * otherwise (-> slk_gru_backward16_f32 + slk_gemm_bf16x6_f32 on da).  yref (or NULL): the OUTPUT of the element-wise activation `dact`
 * whose result is this layer's input, rows ldyref apart -- dx then leaves multiplied by fun'(.), i.e. as dL/d(pre-activation) of the
 * layer below (what slk_gemm_dact_bf16x6 does for the separate product). */
SLK_API int slk_gru_backward16_dx_f32(const float *dy, long lddy, const float *hprev, long ldhp, const float *zr, const float *h,
                              long ldh, const float *sW, const float *sW2, const float *iW, float *da, float *rh, float *dx,
                              long lddx, int T, int B, int n, int insize, int reverse, int act, int gate_act, const float *yref,
                              long ldyref, int dact, slk_stream_t stream);
/* Lstm (layers.py:677-697) in the reverse pass.  sum:[M][4n] = [x_t | out_{t-1}] . [iW | sW]^T + b (a GEMM over
 * slk_train_pack_xh_f32 rows), gate rows interleaved j*4 + gate as the reference stores them.
 *   slk_lstm_gates_f32: the element-wise cell recursion -> gates:[M][4n] = (candidate, input, forget, output) activated,
 *     cell:[M][n] = c_t.   peep:[3][n] or NULL.
 *   slk_lstm_backward_f32: the reverse scan -> dsum:[M][4n] = dL/dsum, dpeep:[B][3][n] per-chunk peephole gradients.
 *     n in {16,32,48,64,96,128}, tanh / sigmoid.  Then diW = dsum^T x, dsW = dsum^T out_prev, db = dsum^T 1, dx = dsum . iW. */
SLK_API int slk_lstm_gates_f32(const float *sum, const float *peep, float *gates, float *cell, int T, int B, int n, int reverse,
                       slk_stream_t stream);
SLK_API int slk_lstm_backward_f32(const float *dy, long lddy, const float *gates, const float *cell, const float *sW, const float *peep,
                          float *dsum, float *dpeep, int T, int B, int n, int reverse, int act, int gate_act,
                          slk_stream_t stream);
/* The same reverse scan on the barrier-stepped fp16-split plan of csrc/lstm_scan16.hip (csrc/lstm_bwd16.hip: n a multiple of 16 up to
 * 64, tanh / sigmoid, gates / dsum 16-byte aligned, operands < 4 GiB; SLK_ERR_UNSUPPORTED otherwise -> slk_lstm_backward_f32). */
SLK_API int slk_lstm_backward16_f32(const float *dy, long lddy, const float *gates, const float *cell, const float *sW, const float *peep,
                          float *dsum, float *dpeep, int T, int B, int n, int reverse, int act, int gate_act,
                          slk_stream_t stream);
SLK_API int slk_softmax_xent_grad_f32(float *logits, long ld, const float *stats, const int32_t *labels, const float *weights, int T,
                              int B, int nstate, int drop, float min_prob, float *loss_rows, float *correct_rows,
                              slk_stream_t stream);
/* The sequence loss in the same place (csrc/seq_loss.hip, design/sequence_loss.md): dL/dlogits of L = -sum_b chunk_scale[b] * ll_b,
 * ll_b the forward score of chunk b's sequence under min_prob + (1 - min_prob) softmax(logits), in place over the logits written by
 * slk_linear_rowstats_* (stats:[M][2] = max, 1/sum).  occ:[T][B] rows of occ_ld floats and score:[B] are what
 * slk_forward_backward_batch_f32 wrote for that posterior in the network layout (row_step = B) with the same min_prob.  Per row
 * m = t*B + b:  p = exp(l - max) / sum, p' = min_prob + (1 - min_prob) p, w = occ (1 - min_prob) p / p' (0 where occ is 0),
 * l_k <- -chunk_scale[b] (w_k - p_k sum_j w_j) for k < nstate; columns nstate..ld-1 are set to zero and nothing else is written.
 * Every row of a chunk whose score is not finite (NaN: refused, its occ was never written and is not read here; -inf: no alignment)
 * becomes exact zeros, columns 0..ld-1.  A row's result depends on that row, score[b] and chunk_scale[b] only: the sum over j runs
 * in a fixed order (per lane ascending columns, then the wave's xor tree), the same at every alignment and batch size.
 * nstate >= 2, ld >= nstate, occ_ld >= nstate, 0 <= min_prob < 1, else SLK_ERR_INVALID_ARG; rows of more than SLK_SEQ_GRAD_MAX_LD
 * floats (or more than 2^33 rows): SLK_ERR_UNSUPPORTED.  16-byte accesses where ld (occ_ld) is a multiple of 4 and the base is
 * 16-byte aligned; rows of up to 2048 floats are read once. */
#define SLK_SEQ_GRAD_MAX_LD (1L << 24)
SLK_API int slk_softmax_seq_grad_f32(float *logits, long ld, const float *stats, const float *occ, long occ_ld, const double *score,
                             const float *chunk_scale, int T, int B, int nstate, float min_prob, slk_stream_t stream);
/* The softmax layer of a training step WITHOUT a logits tensor: the layer's products (pre-split weights, as for
 * slk_linear_rowstats_f16x3) are computed twice -- a statistics pass that stores nothing but, per row, the loss term, the accuracy
 * term and four floats in xrow:[M][4], and a gradient pass that stores grad:[M][ld] = dL/dlogits (columns N..ld-1 zero) -- instead
 * of written, read, overwritten and read again.  Same values bit for bit as slk_linear_rowstats_f16x3 followed by
 * slk_softmax_xent_grad_f32.  M = T * B; K in 49..64 or 81..128, N <= 2048, ld <= N rounded up to 64, xrow 16-byte aligned;
 * SLK_ERR_UNSUPPORTED otherwise (-> the two calls above). */
SLK_API int slk_linear_xent_grad_f16x3(const float *x, long ldx, const void *W_hi, const void *W_lo, const float *W_inv_scale,
                               const float *bias, float *grad, long ld, int K, int N, const int32_t *labels, const float *weights,
                               int T, int B, int drop, float min_prob, float *loss_rows, float *correct_rows, float *xrow,
                               slk_stream_t stream);
SLK_API int slk_reduce_sum_f32(const float *x, size_t n, int square, double *out, slk_stream_t stream);
/* out[r] = sum of x[r][0..n) for r < nrow (<= 16) contiguous arrays, float64, fixed order, 256 workgroups per array (the loss and
 * accuracy terms of a step: two launches of ~5 us where two slk_reduce_sum_f32 take 2 x 74 us).  scratch: nrow * 256 doubles. */
SLK_API int slk_reduce_rows_sum_f32(const float *x, int nrow, size_t n, double *out, double *scratch, slk_stream_t stream);
/* The Softmax layer of a VALIDATION batch (bin/validate_network.py:46-54), forward only.  Per row m of the M = T * B rows:
 * loss_rows[m] = -log p[m, labels[m]] (float32, undivided; no min_prob, drop or weights) and correct_rows[m] = 1 (int32) where the
 * FIRST column that attains the row maximum is the label (T.argmax's rule), else 0.
 *   slk_linear_xent_eval_f16x3: from the layer's input, the statistics pass of slk_linear_xent_grad_f16x3 alone -- no logits, no
 *     gradient, no scratch; at min_prob = 0, drop = 0 and unit weights the training entry point's loss term is this one divided by M,
 *     same bits.  Shapes as there (K in 49..64 or 81..128, N <= 2048), SLK_ERR_UNSUPPORTED otherwise (-> the next one).  A label
 *     outside [0, N) matches no column: garbage loss for that row, no access out of bounds.
 *   slk_softmax_xent_eval_f32: from logits and row statistics written by slk_linear_rowstats_* (read only).  The caller checks that
 *     labels lie in [0, nstate); the kernel clamps the index it reads with.
 *   slk_reduce_rows_sum_i32: out[0] = sum of x[0..n) as a 64-bit integer (the count of correct positions). */
SLK_API int slk_linear_xent_eval_f16x3(const float *x, long ldx, const void *W_hi, const void *W_lo, const float *W_inv_scale,
                               const float *bias, int K, int N, const int32_t *labels, int T, int B, float *loss_rows,
                               int32_t *correct_rows, slk_stream_t stream);
SLK_API int slk_softmax_xent_eval_f32(const float *logits, long ld, const float *stats, const int32_t *labels, int T, int B, int nstate,
                              float *loss_rows, int32_t *correct_rows, slk_stream_t stream);
SLK_API int slk_reduce_rows_sum_i32(const int32_t *x, size_t n, long long *out, slk_stream_t stream);
SLK_API size_t slk_gemm_tn_workspace_bytes(long M, int N1, int N2);
/* 1..4 contractions over the same M rows in ONE launch (the weight gradients of a recurrent layer all contract the same dL/d(pre-
 * activation) matrix: launched together its rows cross the memory bus once): C[q] = A[q]^T B[q], colsum[q] (the array or an entry may be
 * NULL) = A[q]^T 1.  The arrays have nprob entries and live in host memory.  Six bf16 terms per product as slk_gemm_tn_bf16x6_f32.
 * SLK_ERR_UNSUPPORTED: rows longer than 4 M floats or slices beyond 32-bit byte offsets (-> one slk_gemm_tn_f32 per problem). */
SLK_API size_t slk_gemm_tn_multi_workspace_bytes(long M, int nprob, const int *N1, const int *N2);
SLK_API int slk_gemm_tn_multi_bf16x6_f32(int nprob, const float *const *A, const long *lda, const float *const *B, const long *ldb,
                                 float *const *C, const long *ldc, long M, const int *N1, const int *N2, float *const *colsum,
                                 void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_gemm_tn_f32(const float *A, long lda, const float *B, long ldb, float *C, long ldc, long M, int N1, int N2,
                    float *colsum /* [N1] or NULL */, void *workspace, size_t workspace_bytes, slk_stream_t stream);
/* The same contraction with every float32 operand cut into three bf16 pieces and each product evaluated as six bf16 MFMA terms
 * in float32 accumulators (v_mfma_f32_32x32x16_bf16): float32-grade results (terms below 2^-24 of a product are dropped), no
 * scaling needed (bf16 has float32's exponent range), ~2x the speed of the fp32 MFMA form.  Same workspace.               */
SLK_API int slk_gemm_tn_bf16x6_f32(const float *A, long lda, const float *B, long ldb, float *C, long ldc, long M, int N1, int N2,
                           float *colsum, void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_act_backward_f32(const float *dy, const float *y, float *out, size_t n, int act, slk_stream_t stream);
SLK_API int slk_add_inplace_f32(float *y, const float *x, size_t n, slk_stream_t stream);   /* y += x: dL/dx of Parallel branches */
SLK_API int slk_train_im2col_cin1_f32(const float *x, long x_t_stride, long x_b_stride, int T, int B, int winlen, int stride,
                              int pad_lo, int pad_hi, float *cols, slk_stream_t stream);
/* Any number of input features (a Convolution that is not the first layer, or multi-feature input): x:[T][B][Cin], rows ldx
 * floats apart; cols[(t*B + b)][c*winlen + k] = x(t*stride + k - pad_lo, b, c), zero outside the signal (the flattened column
 * order of Convolution.W:[Cout][Cin][winlen], conv.py:66-111), so dL/dW = dpre^T cols and dL/dcols = dpre . W; col2im is the
 * adjoint (dx(t', b, c) = sum of the dcols entries whose window covers t'), a gather in a fixed order.                     */
SLK_API int slk_train_im2col_f32(const float *x, long ldx, int T, int B, int Cin, int winlen, int stride, int pad_lo, int pad_hi,
                         float *cols, slk_stream_t stream);
SLK_API int slk_train_col2im_f32(const float *dcols, int T, int B, int Cin, int winlen, int stride, int pad_lo, int pad_hi, float *dx,
                         long lddx, slk_stream_t stream);
SLK_API int slk_adamski_update_f32(float *param, const float *grad, float *momentum, float *variance, size_t n, float lr_t,
                           float momentum_decay, float decay1, float decay2, float epsilon, float clip, float l2,
                           float gscale, slk_stream_t stream);
SLK_API int slk_sgd_update_f32(float *param, const float *grad, float *vel, size_t n, float rate, float momentum, float clip,
                       float l2, float gscale, slk_stream_t stream);

/* Read accuracy: what misc/align.py gets from `bwa mem -A 1 -B 2 -O 2 -E 1` (align.py:22) and from pysam's walk over every
 * alignment's CIGAR and NM tag (samacc, align.py:70-133), computed on the device (csrc/align.hip, design/align.md).  This is the
 * OPTIMAL local alignment with affine gaps under those scores (a gap of k letters costs gap_open + k * gap_extend), not bwa's
 * heuristic.  Ties: a gap's opening beats its extension; in a cell the diagonal beats a deletion beats an insertion; a cell whose
 * best is <= 0 is empty; the alignment ends in the cell of greatest score, smallest query index, then smallest reference index.
 *   slk_align_pass_width (host only): P, the reference columns one pass of the kernel covers; references longer than P need the
 *     workspace.
 *   slk_align_local_workspace_bytes: bytes of workspace for B pairs whose queries have at most max_qlen and whose references at most
 *     max_rlen letters (0 when max_rlen <= P, or when a bound is beyond the limit below).
 *   slk_align_local_batch_u8: q:[B][ldq] bytes, row b valid for qlen[b] letters (device int32: what slk_paths_to_bases writes, so a
 *     call's bases are aligned where they lie); r: the references end to end, pair b's at r[roff[b] .. roff[b + 1]) (roff:[B + 1]
 *     device int64).  Letters are compared for equality.  max_qlen / max_rlen (host): upper bounds of the lengths, at most 65535
 *     each -- the counts are carried in 16-bit fields -- SLK_ERR_INVALID_ARG beyond that, as for match or gap_extend < 1, mismatch or
 *     gap_open < 0 or any score > 16384.  A pair whose device-side length exceeds the bound it was launched with is not truncated:
 *     its row is (-1, 0, ...).  out:[B][9] int32 = score, q_start, q_end, r_start, r_end (0-based, half open), match, mismatch,
 *     insertion (query letters against a gap), deletion (reference letters against a gap); all 0 for the empty alignment.
 *   slk_revcomp_u8: out[off[b] + k] = complement(seq[off[b + 1] - 1 - k]) for B packed sequences (off:[B + 1] device int64, max_len
 *     (host) >= the longest); A<->T, C<->G, every other byte unchanged; out must not be seq (the '-' strand of align.py:40-41).    */
SLK_API int slk_align_pass_width(void);
SLK_API size_t slk_align_local_workspace_bytes(int B, int max_qlen, int max_rlen);
SLK_API int slk_align_local_batch_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff, int B,
                                     int max_qlen, int max_rlen, int match, int mismatch, int gap_open, int gap_extend, int32_t *out,
                                     void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_revcomp_u8(const uint8_t *seq, const int64_t *off, int B, long max_len, uint8_t *out, slk_stream_t stream);

/* The columns of those alignments: what a SAM record's CIGAR and an error profile are made of (csrc/align_traceback.hip,
 * design/align_traceback.md).  slk_align_local_batch_u8 keeps no traceback; its row gives the start cell and the numbers of
 * insertions I and deletions D, and relative to its start the alignment never leaves the W = I + D + 1 diagonals i - j in [-D, +I].
 * A second DP over that band alone, anchored at the start cell, under the same tie rules, walks back the same operations.
 *   slk_align_traceback_max_band (host only): the widest band W the kernel accepts.
 *   slk_align_traceback_workspace_bytes (host only): bytes of workspace of ONE pair whose row has the spans q_span = q_end - q_start,
 *     r_span = r_end - r_start and the counts insertion, deletion: 4 bits per band cell, a multiple of 16.  0 for spans and counts
 *     no row can have (negative, beyond 65535, q_span - insertion != r_span - deletion) and for W above the widest band.
 *   slk_align_traceback_batch_u8: q, ldq, qlen, r, roff, B and the four scores as slk_align_local_batch_u8 took them; rows:[B][9]
 *     int32, that call's output, in the coordinates of the `r` it ran against.  Pair b's columns go to ops[ops_off[b] ..
 *     ops_off[b + 1]), one byte per column in query order (SLK_ALIGN_OP_*); ops_off:[B + 1] device int64 with ops_off[b + 1] -
 *     ops_off[b] = match + mismatch + insertion + deletion of the row, ops_bytes (host) the size of `ops`.  Pair b's traceback
 *     bits live in workspace[ws_off[b] .. ws_off[b + 1]) (ws_off:[B + 1] device int64, ws_off[b] a multiple of 16, the slice at
 *     least slk_align_traceback_workspace_bytes of the row; `workspace` 16-byte aligned, workspace_bytes (host) its size).
 *     status:[B] int32: SLK_ALIGN_TB_DONE, SLK_ALIGN_TB_EMPTY (score <= 0: no columns; nothing else of the pair is looked at) or
 *     a negative SLK_ALIGN_TB_* code.  The row is device data and is not trusted: a pair whose spans leave [0, qlen] or
 *     [0, rlen], whose counts are negative or do not add up to the spans, whose band is too wide, whose workspace slice is
 *     misaligned, too short or outside the workspace, or whose ops slice disagrees with its column count is SKIPPED -- nothing
 *     but its row, lengths and offsets is read, nothing but its status written.  SLK_ALIGN_TB_SCORE / _WALK: the band's DP did
 *     not end on the row's score / the walk did not reach the start cell in exactly the announced number of columns (a row that
 *     does not belong to these sequences and scores); the pair's own ops slice may then hold anything.  Nothing outside a
 *     pair's own slices is ever written and no loop bound depends on a score.
 *   slk_align_error_profile_u8: profile:[B][SLK_ALIGN_PROFILE_LEN] int32, every entry written (no zeroing needed; all 0 for a pair
 *     whose status is not SLK_ALIGN_TB_DONE).  Letter classes A, C, G, T, other, gap = 0..5.  Entries 0..35: columns by
 *     query class * 6 + reference class (an insertion has reference class 5, a deletion query class 5; entry 35 stays 0);
 *     36..51: maximal runs of insertions of length 1..15 and >= 16; 52..67: the same for deletions.                              */
#define SLK_ALIGN_OP_MATCH 0
#define SLK_ALIGN_OP_MISMATCH 1
#define SLK_ALIGN_OP_INSERTION 2 /* a query letter against a gap      */
#define SLK_ALIGN_OP_DELETION 3  /* a reference letter against a gap  */
#define SLK_ALIGN_PROFILE_LEN 68
#define SLK_ALIGN_TB_DONE 0
#define SLK_ALIGN_TB_EMPTY 1
#define SLK_ALIGN_TB_BAD_SPAN (-1)  /* a span outside [0, qlen] / [0, rlen], or a length beyond 65535 or the row pitch  */
#define SLK_ALIGN_TB_BAD_COUNT (-2) /* a negative count                                                                  */
#define SLK_ALIGN_TB_BAD_SUM (-3)   /* the spans are not the sums of the counts                                          */
#define SLK_ALIGN_TB_BAND (-4)      /* insertion + deletion + 1 > slk_align_traceback_max_band()                         */
#define SLK_ALIGN_TB_WORKSPACE (-5) /* the pair's workspace slice is misaligned, too short or outside the workspace      */
#define SLK_ALIGN_TB_OPS (-6)       /* the pair's ops slice is not its column count long, or outside `ops`               */
#define SLK_ALIGN_TB_SCORE (-7)     /* the band's DP does not end on the row's score                                     */
#define SLK_ALIGN_TB_WALK (-8)      /* the walk did not reach the start cell in the announced number of columns          */
SLK_API int slk_align_traceback_max_band(void);
SLK_API size_t slk_align_traceback_workspace_bytes(int q_span, int r_span, int insertion, int deletion);
SLK_API int slk_align_traceback_batch_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff, int B,
                                         int match, int mismatch, int gap_open, int gap_extend, const int32_t *rows, uint8_t *ops,
                                         const int64_t *ops_off, size_t ops_bytes, void *workspace, const int64_t *ws_off,
                                         size_t workspace_bytes, int32_t *status, slk_stream_t stream);
SLK_API int slk_align_error_profile_u8(const uint8_t *q, long ldq, const uint8_t *r, const int64_t *roff, const int32_t *rows,
                                       const uint8_t *ops, const int64_t *ops_off, const int32_t *status, int B, int32_t *profile,
                                       slk_stream_t stream);

/* f6. The forward (sum-product) score of a sequence under a transducer posterior: decode.score / decode.forwards
 * (sloika/decode.py:96-139), for `nread` (posterior, sequence) pairs in one launch, one workgroup per pair, in float64
 * (csrc/forward_score.hip, design/forward_score.md).  The score is the reference's up to rounding (it sums in another order and
 * scales by powers of two); a pair's score has the same bits alone, in any batch, in either layout and in any launch.
 *   post: rows of `nstate` probabilities, `ld` >= nstate values apart; row t of pair b is row row_off[b] + t * row_step
 *     (row_off:[nread] device int64).  The network layout [T][B][S] is row_off[b] = b, row_step = B; packed ragged rows are
 *     row_off = ev_off, row_step = 1.  nrow:[nread] device int32, the rows of each pair (0: the score of no rows).
 *   seq:[sum npos] int32 column indices, pair b owns pos_off[b] .. pos_off[b + 1] (pos_off:[nread + 1] device int64); a pair may have
 *     no positions.  max_npos (host): the longest sequence; above slk_forward_score_max_positions() (host only: 8191, the state lives
 *     in registers, 32 values per thread) the call is refused with SLK_ERR_UNSUPPORTED and nothing is written.  A pair longer than
 *     max_npos, or with a symbol that is no column, gets NaN and reads nothing out of bounds.
 *   blank: the column of the stay emission (the reference's is the last, decode.py:131; this project's k-mer transducers have it at
 *     0).  full: decode.py:122-124, 139 (every position must be emitted: -inf when there are more positions than rows).
 *   min_prob (float32 rows only): when > 0 every value read goes through decode.prepare_post's transform first (decode.py:36), the
 *     same bits as slk_prepare_post_f32; must be < 1.  The float64 entry exists so the reference's known answers run unrounded.
 *   score_out:[nread] float64. */
SLK_API int slk_forward_score_max_positions(void);
SLK_API int slk_forward_score_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                        int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                        int full, float min_prob, double *score_out, slk_stream_t stream);
SLK_API int slk_forward_score_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                        int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                        int full, double *score_out, slk_stream_t stream);

/* f6b. Forward-backward over the same recursion: with what probability each row of a pair emits each symbol, summed over all
 * alignments (csrc/forward_backward.hip, design/forward_backward.md).  With f the forward variables of f6 and b their mirror image
 * (b_T = 1, full: e_L; b_{t-1}[j] = b_t[j] p_t[blank] + b_t[j+1] p_t[seq[j]]), row t has stay_t[j] = f_{t-1}[j] p_t[blank] b_t[j],
 * move_t[j] = f_{t-1}[j-1] p_t[seq[j-1]] b_t[j] and z_t their total; occ[t, blank] = sum_j stay_t[j] / z_t and occ[t, c] = the sum
 * of move_t[j] / z_t over the positions that carry c (a symbol equal to `blank` adds to that column).  occ[t, c] = p_t[c] times the
 * derivative of the score by p_t[c]; every row of occ sums to 1.  A pair's results have the same bits alone, in any batch, in either
 * layout, with any ld / occ_ld and in any launch.
 *   post .. min_prob: as for slk_forward_score_batch_*, which refuses what these refuse; in addition nstate <= 8192
 *     (SLK_ERR_UNSUPPORTED: one 64-bit slot per column and row parity lives in LDS).
 *   score:[nread] float64, the bits slk_forward_score_batch_* returns for the same pair.
 *   occ: row t of pair b is row row_off[b] + t * row_step of occ, rows occ_ld >= nstate values apart; float32 for _f32 (the float64
 *     value rounded once), float64 for _f64.  The entry zero-fills columns 0 .. nstate - 1 of the nrow[b] rows of every accepted pair
 *     and writes nothing else; a row whose z_t is 0 or not finite (full with more positions than rows, an end state that underflowed)
 *     stays 0.  May be null.
 *   emit_row:[sum npos] int32, emit_prob:[sum npos] float64, behind pos_off like seq: per position the largest move_t[j] / z_t and the
 *     lowest row that attains it; -1 and 0 for a position that never had a positive value (a pair of no rows among them).  Either may
 *     be null.
 *   A refused pair (longer than max_npos, or a symbol that is no column) gets a NaN score; its occ, emit_row and emit_prob are left
 *     untouched and nothing is read out of bounds.
 *   workspace: 16-byte aligned, slk_forward_backward_workspace_bytes(nread, nrow, pos_off) bytes -- the exact requirement, computed
 *     from HOST copies of nrow and pos_off: the pairs' offsets, then 256 * ppt float64 per row of a pair.  A smaller workspace_bytes
 *     returns SLK_ERR_WORKSPACE and nothing is written.  The entry copies nrow and pos_off to the host to check this, so it
 *     synchronises with `stream` once. */
SLK_API size_t slk_forward_backward_workspace_bytes(int nread, const int32_t *nrow, const int64_t *pos_off);
SLK_API int slk_forward_backward_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           int full, float min_prob, double *score, float *occ, long occ_ld, int32_t *emit_row,
                                           double *emit_prob, void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_forward_backward_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           int full, double *score, double *occ, long occ_ld, int32_t *emit_row, double *emit_prob,
                                           void *workspace, size_t workspace_bytes, slk_stream_t stream);

/* f10. The forward score of edited sequences (csrc/rescore_edits.hip, design/rescore_edits.md): per (posterior, sequence) pair any
 * number of candidate edits "replace positions [start, start + ndel) by these new symbols", each scored as f6 would score the
 * spelled-out sequence with full = 1, up to rounding, at the cost of nrow * (new symbols + 1) cells instead of nrow * npos.  One
 * kernel stores the pair's forward and backward lattices, a second walks every candidate through them.  A candidate's result depends
 * on its pair and on the candidate alone: not on the other candidates, their order, the batch, the layout or the launch.
 *   post .. blank, min_prob: as for slk_forward_backward_batch_* (nstate <= 8192); full is implied, there is no free-end form.
 *   cand_pair, cand_start, cand_ndel:[ncand] device int32: the pair, the first replaced position and how many are replaced.
 *     Candidates come grouped by pair, pairs ascending (SLK_ERR_INVALID_ARG otherwise, or for a pair outside 0 .. nread - 1; nothing
 *     is written); within a pair any order, ascending starts read the workspace best.  A pair may have no candidates; ncand may be 0.
 *   cand_new_off:[ncand + 1] device int64, cand_new: int32 columns: candidate i inserts cand_new[cand_new_off[i] ..
 *     cand_new_off[i + 1]), at most slk_rescore_edits_max_new() = SLK_RESCORE_MAX_NEW of them.  No new symbols: a deletion; ndel = 0:
 *     an insertion.
 *   score:[nread] float64: the pair's own full forward score (f6's value up to rounding; -inf with more positions than rows).
 *   ll_edit:[ncand] float64, in the caller's candidate order; -inf when the edited sequence has more positions than the pair rows.
 *   Refused with NaN, and nothing read out of bounds: a candidate with start < 0, ndel < 0, start + ndel > npos, more than
 *     SLK_RESCORE_MAX_NEW new symbols or a new symbol that is no column (that candidate only); every candidate of a pair that was
 *     itself refused (longer than max_npos, or a symbol that is no column: NaN score, nothing else written for the pair).
 *   workspace: 16-byte aligned, slk_rescore_edits_workspace_bytes(nread, nrow, pos_off) bytes, computed from HOST copies of nrow and
 *     pos_off: two offsets per pair, then 16 (nrow + 1) (ldj + 1) bytes per pair, ldj = npos + 1 rounded up to 2.  A smaller
 *     workspace_bytes returns SLK_ERR_WORKSPACE and nothing is written.  The entry copies nrow, pos_off and cand_pair to the host, so
 *     it synchronises with `stream` once. */
#define SLK_RESCORE_MAX_NEW 8
SLK_API int slk_rescore_edits_max_new(void);
SLK_API size_t slk_rescore_edits_workspace_bytes(int nread, const int32_t *nrow, const int64_t *pos_off);
SLK_API int slk_rescore_edits_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                        int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                        float min_prob, const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                        const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                        double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_rescore_edits_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                        int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                        const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                        const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                        double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream);

/* f10b. f10 for whole reads: banded lattices (csrc/rescore_band.hip, design/rescore_band.md).  A pair keeps `width` states per row
 * instead of all npos + 1: state j exists in row t when band_lo[t] <= j < band_lo[t] + width (and 0 <= j <= npos), every other state
 * counts as 0.  score and ll_edit are then the log-likelihoods summed over the alignments that stay inside the band: never above
 * f10's, and f10's bits when band_lo is all 0 and width > npos.  There is no max_npos: the width chooses the kernel and npos is any
 * int32 up to 2^31 - 16387 (SLK_ERR_UNSUPPORTED above).  Arguments as f10, and
 *   band_lo: device int32, band_off:[nread + 1] device int64: pair b's nrow[b] + 1 entries (one per row index 0 .. nrow[b]) start at
 *     band_off[b].  A valid band has band_lo[0] = 0, no negative entry, does not decrease and ends with band_lo[nrow] + width > npos.
 *     A step may be of any size; one above `width` loses all mass (-inf).
 *   width: 256, 512, 1024 or 2048 (up to slk_rescore_band_max_width()).
 *   SLK_ERR_INVALID_ARG, nothing written: a width that is not built, band_off[b + 1] - band_off[b] != nrow[b] + 1, candidates not
 *     grouped by pair.  NaN per candidate or per pair exactly as f10, and a NaN pair for an invalid band.
 *   An edit's ll_edit is -inf when its column `start` exists in no row of the band, or in none before the last row of column
 *     start + ndel + 1.
 *   workspace: 16-byte aligned, slk_rescore_edits_banded_workspace_bytes(nread, nrow, width) bytes from a HOST copy of nrow: f10's
 *     head, then 16 (nrow + 1) (width + 1) bytes per pair; SLK_ERR_WORKSPACE for less.  The entry copies nrow, pos_off, band_off and
 *     cand_pair to the host, so it synchronises with `stream` once. */
SLK_API int slk_rescore_band_max_width(void);
SLK_API size_t slk_rescore_edits_banded_workspace_bytes(int nread, const int32_t *nrow, int width);
SLK_API int slk_rescore_edits_banded_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                               int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int blank,
                                               float min_prob, const int32_t *band_lo, const int64_t *band_off, int width,
                                               const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                               const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                               double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_rescore_edits_banded_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                               int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int blank,
                                               const int32_t *band_lo, const int64_t *band_off, int width, const int32_t *cand_pair,
                                               const int32_t *cand_start, const int32_t *cand_ndel, const int64_t *cand_new_off,
                                               const int32_t *cand_new, int64_t ncand, double *score, double *ll_edit,
                                               void *workspace, size_t workspace_bytes, slk_stream_t stream);

/* f7. Where on a genome a call lies, and the reference of each read cut from it: the locating half of what misc/align.py gets from
 * `bwa mem -k14 -W20 -r10 ... genome.fa calls.fa` (align.py:46-67) and the cut of misc/get_refs_from_sam.py:40-68, on the device
 * (csrc/genome_map.hip, design/genome_map.md).  A seed-and-vote stage chooses, per query and strand, a band of diagonals; the
 * alignment inside the window that band gives is slk_align_local_batch_u8's, unchanged.  Integer only: no result depends on the order
 * in which anything arrives.  Letters are bytes, A C G T = 0..3, any other byte breaks every k-mer that holds it; a k-mer's code is the
 * base-4 number of its k letters, first letter most significant; k is 8..15 (SLK_ERR_INVALID_ARG otherwise).
 *   slk_genome_kmer_keys_u8: genome:[G] bytes, the contigs end to end, contig c at contig_off[c] .. contig_off[c + 1] (contig_off:
 *     [ncontig + 1] device int64, ascending, contig_off[ncontig] = G; ncontig >= 1); G < 2^31 (host), SLK_ERR_INVALID_ARG beyond.
 *     keys:[G] int64, keys[p] = code << 32 | p; a k-mer that holds another byte, crosses its contig's end or runs past G has the code
 *     field 0x7FFFFFFF, so that it sorts behind every real code.  nvalid: one device int32, set to the number of real codes (the
 *     entry zeroes it first).  The caller sorts `keys` ascending (they are distinct: the order is unique) before the next entry.
 *   slk_genome_seed_workspace_bytes: bytes of workspace for B queries of at most max_qlen letters on a genome of G letters: per
 *     workgroup one int32 per bin and two per query position, for min(2 B, 2048) workgroups or as many as fit in 4 GiB (at least
 *     one); 0 for B = 0 or a shape the entry below refuses.  The entry takes any workspace that holds one workgroup's share and
 *     launches as many workgroups as the workspace it is given holds.
 *   slk_genome_seed_votes_u8: q:[B][ldq] bytes, row b valid for qlen[b] letters (device int32: the buffer slk_paths_to_bases writes);
 *     keys: the SORTED keys, of which the first nvalid (host) are real.  For each query, strand s (0: the query; 1: its reverse
 *     complement, formed from the same letters) and position i with a valid k-mer: its occurrences in the genome -- none of them
 *     when there are more than max_occ (1..4096) -- each at p give the diagonal D = p - i + 65536, counted in the bins D / bin_width
 *     and D / bin_width - 1 (bin b covers the diagonals [b W, (b + 2) W)).  bin_width: a power of two, 2..32768, and
 *     max_qlen + bin_width <= 65536 (then D >= bin_width and no bin is negative); SLK_ERR_INVALID_ARG otherwise, as for
 *     max_qlen > 65535 or ldq < max_qlen.  out:[B][2][4] int32 = bin (greatest count; ties go to the smallest bin; 0 without a vote),
 *     votes (that count), second (the greatest count among bins further than 2 from `bin`), nseed (valid k-mers not skipped for
 *     max_occ).  A query shorter than k or without a valid k-mer has votes = 0.  A query whose device-side length is negative or
 *     exceeds max_qlen is not truncated: bin = -1 on both strands.  workspace: 4-byte aligned, SLK_ERR_WORKSPACE when it holds less
 *     than one workgroup's share; its contents on entry do not matter (a workgroup zeroes its share, and leaves it zero).
 *   slk_genome_windows_u8: for B half-open spans [start[b], end[b]) of the genome (device int64) writes the span -- or, where
 *     minus[b] != 0 (device int32), its reverse complement, by slk_revcomp_u8's rule: A<->T, C<->G, every other byte unchanged -- to
 *     out[out_off[b] ..], end to end: out_off:[B + 1] device int64 with out_off[b + 1] - out_off[b] = end[b] - start[b], so `out` and
 *     `out_off` are the aligner's r / roff as they lie, and the per-read references of get_refs_from_sam.py:57-64.  max_len (host) >=
 *     the longest span.  A span that is not inside [0, G], or whose length disagrees with out_off, is skipped: nothing is read or
 *     written for it.  out must not be genome.                                                                                   */
SLK_API int slk_genome_kmer_keys_u8(const uint8_t *genome, const int64_t *contig_off, int ncontig, long G, int k, int64_t *keys,
                                    int32_t *nvalid, slk_stream_t stream);
SLK_API size_t slk_genome_seed_workspace_bytes(int B, int max_qlen, long G, int bin_width);
SLK_API int slk_genome_seed_votes_u8(const uint8_t *q, long ldq, const int32_t *qlen, int B, int max_qlen, const int64_t *keys,
                                     int nvalid, long G, int k, int bin_width, int max_occ, int32_t *out, void *workspace,
                                     size_t workspace_bytes, slk_stream_t stream);
SLK_API int slk_genome_windows_u8(const uint8_t *genome, long G, const int64_t *start, const int64_t *end, const int32_t *minus,
                                  const int64_t *out_off, int B, long max_len, uint8_t *out, slk_stream_t stream);

/* f9. The alignments of f7 / f8 on top of each other: counts per position of the packed genome and the consensus they give
 * (csrc/pileup.hip; design/pileup.md section 1 DEFINES the forward view, the left-normalisation of gaps, the tables and the call, and
 * is not repeated here).  Integer only; the tables are added to with integer atomics, so they depend on no launch shape or order.
 *   slk_pileup_columns_u8: q, ldq, qlen, r, roff, rows, ops, ops_off, ops_bytes as slk_align_traceback_batch_u8 took and left them,
 *     tb_status its status.  minus:[B] device int32 (non-zero: the pair was aligned against the reverse-complemented window), keep:[B]
 *     device bytes, t0:[B] device int64, the packed-genome position of the forward view's first reference letter, G (host) the packed
 *     genome's length.  fcodes: a buffer of ops_bytes bytes that does not overlap `ops`; pair b's forward view goes to
 *     fcodes[ops_off[b] .. ops_off[b + 1]), left-normalised when normalise != 0.  status:[B] int32: SLK_PILEUP_DONE,
 *     SLK_PILEUP_SKIPPED (keep[b] == 0, or tb_status[b] is not SLK_ALIGN_TB_DONE: nothing else of the pair is looked at) or a
 *     negative SLK_PILEUP_* code.  Rows and codes are device data and are not trusted: a pair whose spans leave [0, qlen] /
 *     [0, rlen] (lengths beyond 65535 or the row pitch included), whose counts are negative or do not add up to the spans, whose ops
 *     slice is not its column count long or lies outside ops_bytes, whose t0 is negative or has t0 + r_span > G, that holds a code
 *     byte above 3, or whose codes of a kind are not as many as its row says is REFUSED: nothing but its status is written, its
 *     slice of fcodes is left as it was.  No loop bound depends on a value that has not passed these checks.
 *   slk_pileup_count_u8: adds the pairs whose status (the array above) is SLK_PILEUP_DONE into counts:[hi - lo][8] and
 *     ins:[hi - lo][max_ins][5] int32, the tables of packed positions [lo, hi), 0 <= lo <= hi <= G, max_ins 1..SLK_PILEUP_MAX_INS
 *     (SLK_ERR_INVALID_ARG otherwise).  The caller zeroes the tables once; calls only ever add.  counts entries: 0..3 A C G T of a
 *     query letter aligned to the position (of the forward strand: a '-' pair's letters are complemented), 4 another query letter,
 *     5 deletion, 6 SLK_PILEUP_INS_READS reads with an insertion directly behind the position, 7 SLK_PILEUP_SPAN reads whose
 *     alignment covers this reference letter and the next.  ins[p][k][c]: class c of the k-th letter of an insertion behind p, k <
 *     max_ins.  Columns outside [lo, hi) are walked and not counted.  The rows are checked again (a pair that fails adds nothing): no
 *     read depends on the status array being the one the first entry wrote.
 *   slk_pileup_call_u8: per position of [lo, hi) the call of section 1.4 from the two tables and genome:[G]: letters:[hi - lo][1 +
 *     max_ins] bytes of which the first nlet[p] (0 .. 1 + max_ins) are the position's part of the consensus and the rest 0,
 *     flags:[hi - lo] bytes of SLK_PILEUP_FLAG_*.  A position whose depth (entries 0..5) is under min_depth, or that has no A, C, G, T
 *     or deletion, keeps the genome's byte and gets SLK_PILEUP_FLAG_LOW.  counts must be 16-byte aligned.                        */
#define SLK_PILEUP_MAX_INS 16
#define SLK_PILEUP_INS_READS 6
#define SLK_PILEUP_SPAN 7
#define SLK_PILEUP_FLAG_LOW 1
#define SLK_PILEUP_FLAG_CHANGED 2  /* a substitution or a deletion against the reference letter */
#define SLK_PILEUP_FLAG_INSERTED 4
#define SLK_PILEUP_DONE 0
#define SLK_PILEUP_SKIPPED 1
#define SLK_PILEUP_BAD_SPAN (-1)   /* a span outside [0, qlen] / [0, rlen], or a length beyond 65535 or the row pitch   */
#define SLK_PILEUP_BAD_COUNT (-2)  /* a negative count                                                                   */
#define SLK_PILEUP_BAD_SUM (-3)    /* the spans are not the sums of the counts                                           */
#define SLK_PILEUP_OPS (-4)        /* the pair's ops slice is not its column count long, or outside `ops`                */
#define SLK_PILEUP_POSITION (-5)   /* t0 < 0 or t0 + r_span > G                                                          */
#define SLK_PILEUP_BAD_CODE (-6)   /* a code byte above 3                                                                */
#define SLK_PILEUP_CODE_COUNT (-7) /* the columns of a kind are not as many as the row says                              */
SLK_API int slk_pileup_columns_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff,
                                  const int32_t *rows, const uint8_t *ops, const int64_t *ops_off, size_t ops_bytes,
                                  const int32_t *tb_status, const int32_t *minus, const uint8_t *keep, const int64_t *t0, long G, int B,
                                  int normalise, uint8_t *fcodes, int32_t *status, slk_stream_t stream);
SLK_API int slk_pileup_count_u8(const uint8_t *q, long ldq, const int32_t *qlen, const int64_t *roff, const int32_t *rows,
                                const uint8_t *fcodes, const int64_t *ops_off, size_t ops_bytes, const int32_t *status,
                                const int32_t *minus, const int64_t *t0, long G, int B, long lo, long hi, int max_ins, int32_t *counts,
                                int32_t *ins, slk_stream_t stream);
SLK_API int slk_pileup_call_u8(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G, long lo, long hi, int max_ins,
                               int min_depth, uint8_t *letters, uint8_t *nlet, uint8_t *flags, slk_stream_t stream);

/* f9, quality-weighted (design/pileup.md section 9 DEFINES the weight of a letter and of a column, the weighted tables and the
 * weighted call, and is not repeated here).  Integer only.
 *   slk_pileup_count_qual_u8: slk_pileup_count_u8 with qual:[B][ldq] device bytes (one quality byte per query letter, the pitch of q)
 *     and weights:[256] device bytes.  Adds into counts / ins exactly what slk_pileup_count_u8 adds for the same input (one kernel
 *     text) and, in the same pass, each column's weight into wcounts:[hi - lo][8] and wins:[hi - lo][max_ins][5] int32 (caller-zeroed,
 *     only added to; same indices).  Any byte indexes `weights`, so qual needs no check.  Sums stay below 2^31 for depths up to 8.4
 *     million (255 a letter at the most).  A pair whose row fails the checks adds nothing to any of the four tables.  A null qual,
 *     weights, wcounts or wins gives SLK_ERR_INVALID_ARG.
 *   slk_pileup_call_qual_u8: the weighted call per position of [lo, hi): the winner by weight (depth, for min_depth, is the plain one
 *     of counts), letters / nlet / flags as slk_pileup_call_u8 writes them, letq:[hi - lo][1 + max_ins] the quality of every emitted
 *     letter (unused slots 0) and posq:[hi - lo] the winner's lead over the runner-up, 0 .. qmax, written for a deletion too.  qmax
 *     outside 1..93 gives SLK_ERR_INVALID_ARG.  counts and wcounts must be 16-byte aligned.                                      */
SLK_API int slk_pileup_count_qual_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *qual, const int64_t *roff,
                                     const int32_t *rows, const uint8_t *fcodes, const int64_t *ops_off, size_t ops_bytes,
                                     const int32_t *status, const int32_t *minus, const int64_t *t0, long G, int B, long lo, long hi,
                                     int max_ins, const uint8_t *weights, int32_t *counts, int32_t *ins, int32_t *wcounts,
                                     int32_t *wins, slk_stream_t stream);
SLK_API int slk_pileup_call_qual_u8(const int32_t *counts, const int32_t *ins, const int32_t *wcounts, const int32_t *wins,
                                    const uint8_t *genome, long G, long lo, long hi, int max_ins, int min_depth, int qmax,
                                    uint8_t *letters, uint8_t *nlet, uint8_t *flags, uint8_t *letq, uint8_t *posq,
                                    slk_stream_t stream);

/* f10c. The genome half and the signal half joined (csrc/polish_genome.hip; design/polish_genome.md section 1 DEFINES the row span, the
 * window, the centre line, the candidates' order and triples and the sum, and is not repeated here).
 *   slk_polish_read_windows: one wave per read.  paths:[B][ldp], lens:[B], move_row:[B][ldm] as slk_viterbi_marginals_f32 left them
 *     (T: the entries a row may hold, T <= ldp, ldm), nrow:[B] the posterior rows of each read; qlen, ldq, roff, rows, ops, ops_off,
 *     ops_bytes, tb_status as slk_align_traceback_batch_u8 took and left them (window coordinates; a '-' read against the
 *     reverse-complemented window); minus, keep as slk_pileup_columns_u8; wstart:[B] int64 the packed-genome position of the
 *     mapping window's first forward letter, coff:[B] int64 the packed position of the read's contig, G the packed genome's length.
 *     letter_row:[B][ldq] int32 work table: the posterior row of every called letter (the move_row of the k-mer that emitted it, by
 *     the overlap rule of slk_paths_to_bases with always_move = 1).  Out, for a read with status SLK_POLISH_DONE only: row_span:
 *     [B][2] int32 the rows [r0, r1) of the aligned part, window:[B][2] int64 the draft window [w0, w1) in CONTIG coordinates, and
 *     r1 - r0 + 1 int32 entries at center + center_off[b] (center_off:[B + 1] device int64; a slice too short: SLK_POLISH_CENTER).
 *     status:[B] int32: SLK_POLISH_DONE, SLK_POLISH_SKIPPED (keep[b] == 0 or tb_status[b] is not SLK_ALIGN_TB_DONE: nothing else of
 *     the read is looked at) or a negative SLK_POLISH_* code.  Everything is device data and is not trusted: a refused read gets
 *     its status and nothing else (its slice of the work table apart); no loop bound depends on a value that has not been checked.
 *   slk_letter_edits_count: nwin windows (win_off: the packed position of the window's contig, [w0, w1) in contig coordinates; all
 *     device int64) -> ncand:[nwin + 1], nkmer:[nwin + 1] int64 with entry 0 zero and entry b + 1 the candidates and the k-mers of
 *     window b (0 for a window that is no span of the genome).  An inclusive prefix sum in place makes them cand_off and pos_off.
 *     kmer_len 3 .. SLK_RESCORE_MAX_NEW - 1; kinds: bit 0 substitutions, bit 1 deletions, bit 2 insertions; margin >= 0.
 *   slk_letter_edits_emit: per candidate cand_pair (its window), cand_start, cand_ndel, cand_edit = 8 * packed forward position +
 *     slot, and the NUMBER of its new symbols in cand_new_off[i + 1] (cand_new_off[0] = 0): an inclusive prefix sum in place makes
 *     cand_new_off.  minus:[nwin] device int32: the window is the reverse complement of its span.  A window whose share of cand_off
 *     is not its own count is not followed: its candidates get start -1, which the scoring entries refuse with NaN.
 *   slk_letter_edits_new: the new symbols (posterior columns: state + (state >= blank)) behind the summed cand_new_off; new_cap: the
 *     entries cand_new holds (ncand * (kmer_len + 1) always suffices).  A k-mer with a letter that is none of A C G T is column -1.
 *   slk_polish_window_kmers: seq:[npos] int32, the windows' own k-mer columns behind pos_off:[nwin + 1].
 *   slk_polish_sum_gains_f64: order:[ncand] device int64, the candidates sorted by (cand_edit, cand_pair) -- the caller's sort.  Adds
 *     into gain:[P][8] float64 and support:[P][8] int32, the cells of packed positions [region_start, region_start + P): per cell,
 *     continuing from what it holds, ll_edit - score[cand_pair] of its candidates in that order when both are finite, and their
 *     number; a NaN ll_edit or score makes the cell NaN.  One thread walks a cell: no floating-point atomics, no bit depends on the
 *     launch.  The caller zeroes the tables once; launches that come in read order give the bits of one launch.                    */
#define SLK_POLISH_DONE 0
#define SLK_POLISH_SKIPPED 1
#define SLK_POLISH_BAD_SPAN (-1)   /* a span outside [0, qlen] / [0, rlen], or a length beyond 65535 or the row pitch   */
#define SLK_POLISH_BAD_COUNT (-2)  /* a negative count                                                                   */
#define SLK_POLISH_BAD_SUM (-3)    /* the spans are not the sums of the counts                                           */
#define SLK_POLISH_OPS (-4)        /* the read's ops slice is not its column count long, or outside `ops`                */
#define SLK_POLISH_POSITION (-5)   /* the mapping window is not inside the genome, or in front of its contig             */
#define SLK_POLISH_BAD_CODE (-6)   /* a code byte above 3                                                                */
#define SLK_POLISH_CODE_COUNT (-7) /* the columns of a kind are not as many as the row says                              */
#define SLK_POLISH_PATH (-8)       /* no call, a state that is no k-mer, or letters that are not as many as qlen says    */
#define SLK_POLISH_MOVE_ROW (-9)   /* a move_row outside the read's rows, or one that decreases                          */
#define SLK_POLISH_SHORT (-10)     /* the aligned window has no k-mer                                                    */
#define SLK_POLISH_FEW_ROWS (-11)  /* the aligned part has fewer rows than the window has k-mers                         */
#define SLK_POLISH_CENTER (-12)    /* the read's slice of `center` is shorter than its rows + 1                          */
SLK_API int slk_polish_read_windows(const int32_t *paths, long ldp, const int32_t *lens, const int32_t *move_row, long ldm, int T,
                                    const int32_t *nrow, const int32_t *qlen, long ldq, const int64_t *roff, const int32_t *rows,
                                    const uint8_t *ops, const int64_t *ops_off, size_t ops_bytes, const int32_t *tb_status,
                                    const int32_t *minus, const uint8_t *keep, const int64_t *wstart, const int64_t *coff, long G,
                                    int B, int kmer_len, const int64_t *center_off, int32_t *letter_row, int32_t *status,
                                    int32_t *row_span, int64_t *window, int32_t *center, slk_stream_t stream);
SLK_API int slk_letter_edits_count(const int64_t *win_off, const int64_t *w0, const int64_t *w1, int nwin, long G, int kmer_len,
                                   int kinds, int margin, int64_t *ncand, int64_t *nkmer, slk_stream_t stream);
SLK_API int slk_letter_edits_emit(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                  const int32_t *minus, int nwin, int kmer_len, int kinds, int margin, const int64_t *cand_off,
                                  int64_t ncand, int32_t *cand_pair, int32_t *cand_start, int32_t *cand_ndel, int64_t *cand_new_off,
                                  int64_t *cand_edit, slk_stream_t stream);
SLK_API int slk_letter_edits_new(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                 const int32_t *minus, int nwin, int kmer_len, int blank, int kinds, int margin,
                                 const int64_t *cand_off, int64_t ncand, const int32_t *cand_start, const int64_t *cand_new_off,
                                 int64_t new_cap, int32_t *cand_new, slk_stream_t stream);
SLK_API int slk_polish_window_kmers(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                    const int32_t *minus, int nwin, int kmer_len, int blank, const int64_t *pos_off, int64_t npos,
                                    int32_t *seq, slk_stream_t stream);
SLK_API int slk_polish_sum_gains_f64(const double *score, int nread, const double *ll_edit, const int32_t *cand_pair,
                                     const int64_t *cand_edit, const int64_t *order, int64_t ncand, int64_t region_start, int64_t P,
                                     double *gain, int32_t *support, slk_stream_t stream);

/* f10d. Proposed variants of any length on genome coordinates (csrc/polish_variants.hip; design/polish_variants.md section 1 DEFINES
 * the variant, a window's candidates and their order, the triple, the sum and the repeat-unit proposals, and is not repeated here).
 *   A variant list is var_off:[V] int64 (the packed position of the variant's contig), var_pos:[V] int64 (within the contig),
 *     var_ndel:[V] int32, var_alt_off:[V + 1] int64 into var_alt:[A] uint8 letters, SORTED by (var_off, var_pos); contig_off:
 *     [ncontig + 1] device int64, the contigs' packed starts and G.  All of it is device data and is not trusted: no address and no
 *     loop bound depends on an unchecked value (a list that is not sorted gives some of its fitting variants, never a bad access).
 *   slk_variant_edits_count: var_status:[V] int32 <- SLK_VARIANT_OK or a negative SLK_VARIANT_* code; a refused variant gets no
 *     candidate anywhere and nothing of it is read beyond the check.  Then, one wave per window (win_off, w0, w1 as
 *     slk_letter_edits_count), ncand:[nwin + 1] and nkmer:[nwin + 1] int64 with entry 0 zero and entry b + 1 the candidates (the
 *     variants of the window's contig with w0 + margin <= var_pos, var_pos + var_ndel <= w1 - margin and a k-mer left) and the k-mers
 *     of window b.  An inclusive prefix sum in place makes them cand_off and pos_off.  kmer_len 3 .. SLK_RESCORE_MAX_NEW - 1.
 *   slk_variant_edits_emit: one wave per window, the count pass's walk; per candidate cand_pair (its window), cand_start, cand_ndel,
 *     cand_var (the index into the sorted list) and the NUMBER of its new symbols in cand_new_off[i + 1] (cand_new_off[0] = 0).
 *     Within a '+' window by ascending variant, within a '-' window (minus:[nwin] int32) by descending.  Entries of a window's share
 *     of cand_off beyond its own count get start -1 and cand_var -1, which the scoring entries refuse with NaN.
 *   slk_variant_edits_new: one thread per candidate, the new symbols (posterior columns, state + (state >= blank); -1 for a k-mer with
 *     a letter that is none of A C G T) behind the summed cand_new_off; new_cap: the entries cand_new holds (ncand *
 *     SLK_RESCORE_MAX_NEW always suffices).  The windows' own columns are slk_polish_window_kmers'.
 *   slk_polish_sum_variant_gains_f64: order:[ncand] device int64, the candidates sorted by (cand_var, cand_read) -- the caller's sort;
 *     read_minus:[nread] int32.  Adds into gain, support, pro:[V] and gain_strand, support_strand, pro_strand:[V][2] ('+' 0, '-' 1 by
 *     the scoring read's strand): per cell, continuing from what it holds, ll_edit - score[cand_read] of its candidates in that order
 *     when both are finite, their number, and how many were > 0; a NaN of either value makes the total's and that strand's gain NaN.
 *     One thread walks a variant: no floating-point atomics, no bit depends on the launch.
 *   slk_repeat_variants_count / _emit: one thread per packed position of [lo, lo + P).  nprop, nalt:[P + 1] int64 with entry 0 zero
 *     and entry t + 1 the proposals and their alt letters at position lo + t; summed in place they are prop_off and alt_off, and the
 *     emit pass writes the V = prop_off[P] variants and A = alt_off[P] letters in the list's layout, sorted as they come.  max_unit
 *     1 .. 4, max_change 1 .. 8, min_copies >= 2.  Offsets that are not a position's own counts are not followed.                   */
#define SLK_VARIANT_OK 0
#define SLK_VARIANT_CONTIG (-1)    /* var_off is no contig's start                                                       */
#define SLK_VARIANT_SPAN (-2)      /* var_pos negative, or [var_pos, var_pos + var_ndel) not inside the contig           */
#define SLK_VARIANT_NDEL (-3)      /* a negative var_ndel                                                                */
#define SLK_VARIANT_ALT (-4)       /* the alt slice descends, leaves var_alt or has more than MAX_NEW - kmer_len + 1     */
#define SLK_VARIANT_EMPTY (-5)     /* nothing deleted and nothing put in                                                 */
#define SLK_VARIANT_SAME (-6)      /* the alt is the letters that stand there                                            */
SLK_API int slk_variant_edits_count(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, const int64_t *var_off,
                                    const int64_t *var_pos, const int32_t *var_ndel, const int64_t *var_alt_off,
                                    const uint8_t *var_alt, int64_t V, int64_t A, const int64_t *win_off, const int64_t *w0,
                                    const int64_t *w1, int nwin, int kmer_len, int margin, int32_t *var_status, int64_t *ncand,
                                    int64_t *nkmer, slk_stream_t stream);
SLK_API int slk_variant_edits_emit(const uint8_t *genome, long G, const int64_t *var_off, const int64_t *var_pos,
                                   const int32_t *var_ndel, const int64_t *var_alt_off, const uint8_t *var_alt, int64_t V, int64_t A,
                                   const int32_t *var_status, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                   const int32_t *minus, int nwin, int kmer_len, int margin, const int64_t *cand_off, int64_t ncand,
                                   int32_t *cand_pair, int32_t *cand_start, int32_t *cand_ndel, int32_t *cand_var,
                                   int64_t *cand_new_off, slk_stream_t stream);
SLK_API int slk_variant_edits_new(const uint8_t *genome, long G, const int64_t *var_off, const int64_t *var_pos,
                                  const int32_t *var_ndel, const int64_t *var_alt_off, const uint8_t *var_alt, int64_t V, int64_t A,
                                  const int32_t *var_status, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                  const int32_t *minus, int nwin, int kmer_len, int blank, int margin, int64_t ncand,
                                  const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_var,
                                  const int64_t *cand_new_off, int64_t new_cap, int32_t *cand_new, slk_stream_t stream);
SLK_API int slk_polish_sum_variant_gains_f64(const double *score, const int32_t *read_minus, int nread, const double *ll_edit,
                                             const int32_t *cand_read, const int32_t *cand_var, const int64_t *order, int64_t ncand,
                                             int64_t V, double *gain, int32_t *support, int32_t *pro, double *gain_strand,
                                             int32_t *support_strand, int32_t *pro_strand, slk_stream_t stream);
SLK_API int slk_repeat_variants_count(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, int64_t lo, int64_t P,
                                      int kmer_len, int max_unit, int max_change, int min_copies, int64_t *nprop, int64_t *nalt,
                                      slk_stream_t stream);
SLK_API int slk_repeat_variants_emit(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, int64_t lo, int64_t P,
                                     int kmer_len, int max_unit, int max_change, int min_copies, const int64_t *prop_off,
                                     const int64_t *alt_off, int64_t V, int64_t A, int64_t *var_off, int64_t *var_pos,
                                     int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt, slk_stream_t stream);

/* f10e. Alleles proposed by a pileup and genotype log-likelihoods of proposed variants (csrc/genotype.hip; design/genotypes.md section 1
 * DEFINES the test a count passes, what a position proposes and in what order, the skipped bits and the three log-likelihoods, and is
 * not repeated here).  Everything is device data and is not trusted, as in f10d.
 *   slk_pileup_alleles_count / _emit: counts:[P][8] and ins:[P][max_ins][5] int32, the tables of slk_pileup_count_u8 over the packed
 *     positions [lo, lo + P); max_ins 1 .. 16, min_depth >= 1, min_count >= 1, permille 1 .. 1000, max_del 1 .. 2^20.  One thread per
 *     position.  nprop, nalt:[P + 1] int64 with entry 0 zero and entry t + 1 the variants and their alt letters position lo + t
 *     proposes; skipped:[P] int32 <- SLK_ALLELES_SKIPPED_INS where an insertion has more than SLK_RESCORE_MAX_NEW - kmer_len + 1
 *     letters, | SLK_ALLELES_SKIPPED_DEL where a deletion run has more than max_del.  Summed in place nprop and nalt are prop_off and
 *     alt_off, and the emit pass writes the V = prop_off[P] variants and A = alt_off[P] letters in f10d's list layout, sorted as they
 *     come.  Offsets that are not a position's own counts are not followed.
 *   slk_variant_genotypes_f64: score, ll_edit, cand_read, cand_var and order as slk_polish_sum_variant_gains_f64 takes them; scale a
 *     finite double > 0.  Writes gl:[V][3] float64 (0, log-likelihood of 0/1, of 1/1, each against 0/0) and n:[V] int32 of every
 *     variant that has a candidate -- a caller zeroes both first --: per candidate in read order, both values finite,
 *     d = scale * (ll_edit - score[cand_read]), gl1 += max(d, 0) + log1p(exp(-|d|)) - ln 2, gl2 += d, n += 1; a NaN of either value
 *     makes the three NaN.  One thread walks a variant: no floating-point atomics, no bit depends on the launch.                     */
#define SLK_ALLELES_SKIPPED_INS 1
#define SLK_ALLELES_SKIPPED_DEL 2
SLK_API int slk_pileup_alleles_count(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G,
                                     const int64_t *contig_off, int ncontig, int64_t lo, int64_t P, int max_ins, int kmer_len,
                                     int min_depth, int min_count, int permille, int max_del, int64_t *nprop, int64_t *nalt,
                                     int32_t *skipped, slk_stream_t stream);
SLK_API int slk_pileup_alleles_emit(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G,
                                    const int64_t *contig_off, int ncontig, int64_t lo, int64_t P, int max_ins, int kmer_len,
                                    int min_depth, int min_count, int permille, int max_del, const int64_t *prop_off,
                                    const int64_t *alt_off, int64_t V, int64_t A, int64_t *var_off, int64_t *var_pos,
                                    int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt, slk_stream_t stream);
SLK_API int slk_variant_genotypes_f64(const double *score, int nread, const double *ll_edit, const int32_t *cand_read,
                                      const int32_t *cand_var, const int64_t *order, int64_t ncand, int64_t V, double scale, double *gl,
                                      int32_t *n, slk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SLOIKA_AMD_H */
