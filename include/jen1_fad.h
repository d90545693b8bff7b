/*
 * libjen1_hip.so -- the VGGish embedder behind the Frechet Audio Distance: the first layer on the vector ALU, a 3x3 convolution as an
 * implicit GEMM on the exact-float32 matrix instructions, and the ReLU of the linears.  Not in the reference.  csrc/vggish.hip holds
 * the kernels, jen1_amd/fad.py the host side; the linears run on jen1_train_gemm (include/jen1_train.h) and the statistics on
 * jen1_latent_moments (include/jen1_hip.h).
 *
 * Activations are float32 NHWC, [N][H][W][C], H = frames and W = mel bands.  Channel counts are multiples of 16 in 16..512.
 * Every function validates its arguments on the host before anything is launched and returns 0, or non-zero with jen1_last_error()
 * set; `stream` is a hipStream_t.  No atomics, no split over K, one fixed order of every sum: an example's result does not depend on
 * the batch size or on where in the batch it sits.
 */
#ifndef JEN1_FAD_H
#define JEN1_FAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JEN1_VGGISH_FRAMES 96       /* H of an example */
#define JEN1_VGGISH_BANDS 64        /* W of an example */
#define JEN1_CONV3X3_KC 16          /* input channels per staged chunk */
#define JEN1_CONV3X3_BN 64          /* output channels per workgroup */

/* floats of the packed weights of jen1_conv3x3 for (cin, cout); 0 for channel counts the kernel refuses.  The layout, with
 * G = ceil(cout / 64) and Q = cin / 16:
 *   packed[((((g Q + q) 9 + tap) 4 + c4) 4 + nt) 64 + 16 k + j] = w[cout = 64 g + 16 nt + j][cin = 16 q + 4 c4 + k][tap / 3][tap % 3]
 * and zero where 64 g + 16 nt + j >= cout: one (g, q) block is what a workgroup stages per chunk, one run of 64 floats is the B
 * operand of one matrix instruction, lane by lane. */
int64_t jen1_conv3x3_packed_floats(int cin, int cout);

/* y = relu(conv3x3(x, pad 1) + bias), then 2x2 max-pool (stride 2) if pool != 0 (H and W must then be even).
 *   x [N][H][W][cin], packed as above, bias [cout], y [N][H][W][cout] or [N][H / 2][W / 2][cout]; x and y must not overlap. */
int jen1_conv3x3(const float* x, const float* packed, const float* bias, float* y, int N, int H, int W, int cin, int cout, int pool,
                 void* stream);

/* Examples of a batch of rows.  mel: the output of jen1_mel with 64 bands, [rows][64][frames] float32, LINEAR mel.  Example e of row r
 * is the frames [96 e, 96 e + 96) of that row; `counts` is a HOST array [rows] of the examples taken from every row
 * (0 <= 96 counts[r] <= frames); the examples are numbered row by row.
 *
 * out [sum counts][96][64] = log(mel + 0.01), frames by bands. */
int jen1_vggish_examples(const float* mel, const int32_t* counts, int rows, int64_t frames, float* out, void* stream);

/* The first layer on the examples [first, first + n):  y [n][48][32][cout] = maxpool2x2(relu(conv3x3(e) + bias)), w [9][cout]
 * (tap-major), bias [cout].
 *   logmel = 0   src is linear mel as above and e = log(mel + 0.01) is applied where the patch is read
 *   logmel = 1   src is finished log-mel examples [rows][frames][64] (jen1_vggish_examples' layout: rows examples, frames = 96,
 *                every count 1) */
int jen1_vggish_conv1(const float* src, const int32_t* counts, int rows, int64_t frames, int logmel, int64_t first, int64_t n,
                      const float* w, const float* bias, float* y, int cout, void* stream);

/* x[i] = max(x[i], 0) in place, n floats */
int jen1_vggish_relu(float* x, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
