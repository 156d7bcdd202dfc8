// The internal launchers and host helpers of libiunet.so: C++ linkage, typed pointers, hipStream_t.  Each is declared here once, under
// the file that defines it, and nowhere else; default arguments live here only.  common.h includes this header, so the defining file and
// every caller compile against the same declaration.  (The public entry points: include/iunet.h, in the same way.)
#pragma once
#include <hip/hip_runtime.h>

// capi.hip
void iunet_set_error(const char* fmt, ...);

// conv3_host_pack.hip
int iunet_conv3_launch(int dtype, int nd, const void* x, long long x_sstride, void* y, long long y_sstride,
                       const void* wpk, const float* bias, float* stats, int N, int D, int H, int W, int Cin,
                       int Cout, int epi, int layout, hipStream_t stream, const float* in_scale = nullptr,
                       const float* in_shift = nullptr, const void* bw_y = nullptr, long long bw_y_ss = 0,
                       const float* const* bw_par = nullptr);
int iunet_conv3_tiles(int nd, int N, int D, int H, int W);
long long iunet_pack_conv3_size(int Cout, int Cin, int taps, int mode);
int iunet_pack_conv3_launch(int dtype, const float* w, const float* scale, void* dst, int Cout, int Cin, int taps,
                            int mode, hipStream_t stream);

// conv3_v4.hip
int iunet_conv3_v4_launch(int dtype, int nd, const void* x, long long x_sstride, void* y, long long y_sstride, const void* wpk,
                          const float* bias, float* stats, int N, int D, int H, int W, int Cin, int Cout, int epi,
                          const float* in_scale, const float* in_shift, hipStream_t stream, const void* bw_y = nullptr,
                          long long bw_y_ss = 0, const float* const* bw_par = nullptr, int compact = 0, int per_sample = 0,
                          int* query_rows = nullptr);
int iunet_conv3_v4_stats_parts(int nd, int Cout);
int iunet_conv3_v4_pairs(int nd, int N, int D, int H, int W, int Cin, int Cout, int bw);
int iunet_conv3_v4_x2_launch(int nd, const void* x, long long x_sstride, int x_lo, void* y, long long y_sstride, int y_lo, const void* wpk,
                             const float* oscale, const float* bias, int N, int D, int H, int W, int Cin, int Cout, int epi,
                             int* sat, hipStream_t stream);
int iunet_conv3_v4_x2_pack_mode(int nd);

// pointwise.hip
int iunet_first_conv_launch(int dtype, int nd, const void* x, int in_dtype, long long sN, long long sC, long long sD,
                            long long sH, long long sW, void* y, long long y_sstride, const void* w,
                            const float* bias, float* stats, int N, int D, int H, int W, int Cin, int Cout, int relu,
                            hipStream_t stream, int out8 = 0);
int iunet_pack_first_conv_launch(int dtype, const float* w, const float* scale, void* dst, int Cout, int Cin, int taps,
                                 hipStream_t stream);
int iunet_maxpool_launch(int dtype, int nd, const void* x, long long x_ss, void* y, long long y_ss, int planes, int N,
                         int Do, int Ho, int Wo, hipStream_t stream);
int iunet_maxpool_q_launch(int nd, const void* x, long long x_ss, void* y, long long y_ss, int planes16, int N, int Do, int Ho, int Wo,
                           hipStream_t stream);
int iunet_convT_launch(int dtype, int nd, const void* x, long long x_ss, void* y, long long y_ss, const void* wpk,
                       const float* bias, int N, int D, int H, int W, int Cin, int Cout, hipStream_t stream, int out8 = 0);
int iunet_pack_convT_launch(int dtype, const float* w, void* dst, int Cin, int Cout, int npos, hipStream_t stream);
int iunet_head_launch(int dtype, const void* x, long long x_ss, int C0, const float* w, const float* bias, int ncls,
                      float* logits, float* probs, unsigned char* cls, const long long* os, float divisor, int accumulate, int N,
                      int D, int H, int W,
                      hipStream_t stream);

// precise_f32.hip: fp32 parity mode
long long iunet_f32_pack_size(int Cout, int Cin, int taps);
int iunet_f32_pack_launch(const float* w, float* dst, float* bias_out, const float* gamma, const float* beta,
                          const float* mean, const float* var, float eps, int Cout, int Cin, int taps, int transposed,
                          hipStream_t stream);
int iunet_f32_conv_launch(int nd, const void* x, int in_dtype, const long long* st, float* y, long long y_ss, const float* wpk,
                          const float* bias, int N, int D, int H, int W, int Cin, int Cout, int relu, int transposed,
                          hipStream_t stream);
int iunet_f32_maxpool_launch(int nd, const float* x, long long x_ss, float* y, long long y_ss, int C, int N, int Do, int Ho,
                             int Wo, hipStream_t stream);
int iunet_f32_head_launch(const float* x, long long x_ss, int C0, const float* w, const float* bias, int ncls, float* logits,
                          float* probs, unsigned char* cls, const long long* os, float divisor, int accumulate, int N, int D,
                          int H, int W, hipStream_t stream);

// conv3_f8.hip: fp8 matrix-core convolution
long long iunet_f8_pack_bytes(int Cout, int Cin, int taps);
int iunet_f8_pack_launch(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                         void* dst, float* wscale, float* bias_out, int Cout, int Cin, int taps, hipStream_t stream);
long long iunet_conv3_f8_workspace_floats(int nd, int N, int D, int H, int W, int Cin, int Cout);
int iunet_conv3_f8_launch(int dtype, int nd, const void* x, long long x_sstride, void* y, long long y_sstride, const void* wpk,
                          const float* wscale, const float* bias, int N, int D, int H, int W, int Cin, int Cout, int epi,
                          float* workspace, hipStream_t stream);
int iunet_conv3_f8_launch_q(int dtype, int nd, const void* x, long long x_sstride, int x_fmt, void* y, long long y_sstride, int y_fmt,
                            const void* wpk, const float* wscale, const float* bias, int N, int D, int H, int W, int Cin, int Cout,
                            int epi, float* workspace, hipStream_t stream);

// conv3_f8k.hip
int iunet_f8_k128(int taps, int Cin);        // 1 = the K = 128 order (3-D, Cin % 32 == 0), 0 = the K16 order
int iunet_conv3_f8k_launch(int dtype, const void* x, long long x_sstride, void* y, long long y_sstride, const void* wpk,
                           const float* wscale, const float* bias, int N, int D, int H, int W, int Cin, int Cout, int epi,
                           int ksplit, float* partial, int small, int in8, int out8, hipStream_t stream);

// conv3_wgrad_v2.hip, conv2_wgrad_v2.hip
int iunet_conv3_wgrad_v2_blocks(int N, int D, int H, int W, int Cin, int Cout);
int iunet_conv3_wgrad_v2_launch(int dtype, const void* x, long long x_ss, const void* dy, long long dy_ss, float* slab,
                                int N, int D, int H, int W, int Cin, int Cout, const float* x_scale, const float* x_shift,
                                hipStream_t stream);
int iunet_conv2_wgrad_v2_blocks(int N, int H, int W, int Cin, int Cout, int* rows);
int iunet_conv2_wgrad_v2_launch(int dtype, const void* x, long long x_ss, const void* dy, long long dy_ss, float* slab, int N, int H, int W,
                                int Cin, int Cout, const float* x_scale, const float* x_shift, hipStream_t stream);

// train_pointwise.hip: the loss / metrics / coefficient pass that every fused head + loss forward (16-bit, fp32, upsampled) ends with
int iunet_loss_finalize_launch(const float* slab, int nparts, int ncls, int kind, int has_weight, double nvox_total, float* out4,
                               float* coef, hipStream_t stream);
