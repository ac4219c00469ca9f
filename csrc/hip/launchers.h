// The one declaration of every host entry point of the .hip files, grouped by
// the file that defines it.  The bindings include this header and so does
// every .hip file, so each definition is compiled against its declaration.
// Default arguments live here and nowhere else.  No torch, no device code.
#pragma once

#include <hip/hip_runtime.h>

#include "attn_bn.h"

// Conventions: `const void*` / `void*` activations are bf16; an `int x16` flag
// beside one selects bf16 (1) or fp32 (0) at run time.  A trailing `bool acc`
// of a backward launcher says that its parameter-gradient outputs are
// gradient sinks: added to and never cleared.

// ---- edge_attn.hip --------------------------------------------------------
void launch_edge_attn_fwd(const float* q, const float* k, const float* v,
                          const float* e, const int* row_ptr,
                          const int* csr_src, const float* skip, float* out,
                          float* alpha, int n, int h, hipStream_t stream);
void launch_edge_attn_bwd(const float* g, const float* q, const float* k,
                          const float* v, const float* e, const float* alpha,
                          const int* row_ptr, const int* csr_src,
                          const int* col_ptr, const int* csc_eid, float* dq,
                          float* dk, float* dv, float* de, float* dek,
                          float* dev, int n, int h, long num_edges,
                          hipStream_t stream);

// ---- edge_attn_fused.hip --------------------------------------------------
void launch_edge_attn_fused_fwd(const float* qkvs, const float* pifc,
                                const float* prpc, const long* ea, int astride,
                                const int* row_ptr, const int* csr_src,
                                float* out, float* alpha, int n, int h,
                                int heads, hipStream_t stream);
void launch_edge_attn_fused_bwd(const float* g, const float* qkvs,
                                const float* pifc, const float* prpc,
                                const long* ea, int astride,
                                const float* alpha, const int* row_ptr,
                                const int* csr_src, const int* col_ptr,
                                const int* csc_dst, const int* csc_eid,
                                float* dqkvs, float* de, float* dal, int n,
                                int h, long num_edges, int heads,
                                hipStream_t stream);
void launch_edge_attn_fused_fwd16(const void* qkvs, const void* pifc,
                                  const void* prpc, int p16, const long* ea,
                                  int astride, const int* row_ptr,
                                  const int* csr_src, void* out, int out16,
                                  float* alpha, int n, int h, int heads,
                                  hipStream_t stream);
// bn: the BatchNorm backward of g runs inside the row kernel; pool: g is
// formed from the pattern pool's gradient (then the g pointer is null)
void launch_edge_attn_fused_bwd16(const void* g, int g16, const void* qkvs,
                                  const void* pifc, const void* prpc, int p16,
                                  const long* ea, int astride,
                                  const float* alpha, const int* row_ptr,
                                  const int* csr_src, const int* col_ptr,
                                  const int* csc_dst, const int* csc_eid,
                                  void* dqkvs, void* de, float* dal, int n,
                                  int h, long num_edges, int heads,
                                  hipStream_t stream,
                                  const AttnBnBwd* bn = nullptr,
                                  const AttnPoolBwd* pool = nullptr);
void launch_edge_attn_fused_infer(const float* qkvs, const float* pifc,
                                  const float* prpc, const long* ea,
                                  int astride, const int* row_ptr,
                                  const int* csr_src, const float* bn_scale,
                                  const float* bn_shift, int relu, float* out,
                                  int n, int h, int heads,
                                  hipStream_t stream);
void launch_edge_attn_fused_infer16(const void* qkvs, const void* pifc,
                                    const void* prpc, int p16,
                                    const long* ea, int astride,
                                    const int* row_ptr, const int* csr_src,
                                    const float* bn_scale,
                                    const float* bn_shift, int relu,
                                    void* out, int out16, int n, int h,
                                    int heads, hipStream_t stream);

// ---- segops.hip -----------------------------------------------------------
void launch_seg_pool_fwd(const float* x, const float* probs, const float* nn,
                         const int* batch_ptr, float* partial, float* out,
                         int b, int P, int h, hipStream_t stream);
void launch_seg_pool_fwd16(const void* x, const float* probs, const float* nn,
                           const int* batch_ptr, float* partial, float* out,
                           int b, int P, int h, hipStream_t stream);
void launch_seg_pool_bwd(const float* gout, const float* probs,
                         const float* nn, const long* batch, float* dx, long n,
                         int h, hipStream_t stream);
void launch_seg_pool_bwd16(const float* gout, const float* probs,
                           const float* nn, const long* batch, void* dx,
                           long n, int h, hipStream_t stream);
void launch_embed_node_fwd(const float* x_raw, const long* idx,
                           const float* table, float* out, long n, int f,
                           int h, hipStream_t s);
void launch_embed_node_fwd16(const float* x_raw, const long* idx,
                             const float* table, void* out, long n, int f,
                             int h, hipStream_t stream);
void launch_embed_node_pad(const float* x_raw, const long* idx,
                           const float* table, void* out, int out16, long n,
                           int f, int h, int pad_to, hipStream_t s);
void launch_embed_edge_fwd(const long* attr, const float* ifc,
                           const float* rpc, float* out, long e, int h,
                           int astride, hipStream_t s);
void launch_gather_rows(const long* idx, const float* table, float* out,
                        long n, int h, hipStream_t s);
void launch_embed_grouped_scatter(const float* g, const int* order,
                                  const int* ptr, float* partial,
                                  float* dtable, long num_src, int rows, int P,
                                  int h, int gstride, int col_off,
                                  hipStream_t s);
void launch_embed_grouped_scatter_bal(
    const void* g, int g16, const int* order, const int* ptr,
    const int* row_map, const int* wave_start, const int* row_map2,
    const int* wave_start2, float* partial, float* partial2, float* dtable,
    int n_waves, int n_waves2, int rows, int h, int gstride, int col_off,
    hipStream_t s);
void launch_rows_sum_lists(const void* src, int in16, const int* idx,
                           const int* lptr, void* out, int out16, int n_lists,
                           int h, int unroll, hipStream_t s);
void launch_rows_sum_lists_wide(const void* src, int in16, int src_stride,
                                const int* idx, const int* lptr, float* out,
                                int out_stride, int n_lists, int width,
                                int seg_cols, int unroll, hipStream_t s);
void launch_vocab_scatter(const float* g, const long* idx, long idx_stride,
                          float* dtable, long n, int rows, int h, int gstride,
                          int col_off, hipStream_t s);
void launch_vocab_scatter16(const void* g, const long* idx, long idx_stride,
                            float* dtable, long n, int rows, int h,
                            int gstride, int col_off, hipStream_t s);
void launch_vocab_scatter_dual(const float* g, const long* ea, int astride,
                               float* dt0, float* dt1, long n, int rows0,
                               int rows1, int h, hipStream_t s);
void launch_vocab_scatter_dual16(const void* g, const long* ea, int astride,
                                 float* dt0, float* dt1, long n, int rows0,
                                 int rows1, int h, hipStream_t s);

// BatchNorm.  Wide-load path: bn_wide_ok is the fast-path shape test,
// bn_wide_slab_rows the rows of the per-call [rows, 2h] slab a reduction over
// [n, h] needs (0 = none, then `slab` is null).  `mask` is the bit-packed
// ReLU keep mask [n, h/8] of the bf16 forward (or null).
bool bn_wide_ok(int h);
int bn_wide_slab_rows(long n, int h);
void launch_bn_eval_stats(const float* running_mean, const float* running_var,
                          float* mean, float* invstd, int h, float eps,
                          hipStream_t s);
void launch_counter_bump(unsigned long long* c, hipStream_t s);
void launch_bn_grad_affine(const float* partials, float* dgamma, float* dbeta,
                           int h, hipStream_t s, bool acc = false);
void launch_bn_stats_only(const float* x, long n, int h, float* partials,
                          float* slab, hipStream_t s);
void launch_bn_stats_only16(const void* x, long n, int h, float* partials,
                            float* slab, hipStream_t s);
void launch_bn_fwd(const float* x, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* mean,
                   float* invstd, float* partials, float* y, long n, int h,
                   float momentum, float eps, bool training, bool relu,
                   float dropout_p, const unsigned long long* seed_ptr,
                   float* slab, hipStream_t s);
void launch_bn_fwd16(const void* x, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float* mean,
                     float* invstd, float* partials, void* y, long n, int h,
                     float momentum, float eps, bool training, bool relu,
                     float dropout_p, const unsigned long long* seed_ptr,
                     float* slab, unsigned char* mask, hipStream_t s);
void launch_bn_finalize_apply(const float* x, const float* partials,
                              const float* count_ptr, const float* gamma,
                              const float* beta, float* running_mean,
                              float* running_var, float* mean, float* invstd,
                              float* y, long n, int h, float momentum,
                              float eps, bool training, bool relu,
                              float dropout_p,
                              const unsigned long long* seed_ptr,
                              hipStream_t s);
void launch_bn_finalize_apply16(const void* x, const float* partials,
                                const float* count_ptr, const float* gamma,
                                const float* beta, float* running_mean,
                                float* running_var, float* mean, float* invstd,
                                void* y, long n, int h, float momentum,
                                float eps, bool training, bool relu,
                                float dropout_p,
                                const unsigned long long* seed_ptr,
                                unsigned char* mask, hipStream_t s);
void launch_bn_bwd(const float* g, const float* x, const float* y,
                   const float* mean, const float* invstd, const float* gamma,
                   float* partials, float* dx, float* dgamma, float* dbeta,
                   long n, int h, bool relu, float keep_inv, float* slab,
                   hipStream_t s, bool acc = false);
void launch_bn_bwd16(const void* g, const void* x, const void* y,
                     const float* mean, const float* invstd,
                     const float* gamma, float* partials, void* dx,
                     float* dgamma, float* dbeta, long n, int h, bool relu,
                     float keep_inv, float* slab, const unsigned char* mask,
                     hipStream_t s, bool acc = false);
void launch_bn_bwd_partials_only(const float* g, const float* x,
                                 const float* y, const float* mean,
                                 const float* invstd, long n, int h, bool relu,
                                 float* partials, float keep_inv, float* slab,
                                 hipStream_t s);
void launch_bn_bwd_partials_only16(const void* g, const void* x,
                                   const void* y, const float* mean,
                                   const float* invstd, long n, int h,
                                   bool relu, float* partials, float keep_inv,
                                   float* slab, const unsigned char* mask,
                                   hipStream_t s);
void launch_bn_bwd_partials_affine16(const void* g, const void* x,
                                     const unsigned char* mask,
                                     const float* mean, const float* invstd,
                                     long n, int h, float* partials,
                                     float keep_inv, float* slab,
                                     float* dgamma, float* dbeta,
                                     hipStream_t s, bool acc = false);
void launch_bn_bwd_apply_only(const float* g, const float* x, const float* y,
                              const float* mean, const float* invstd,
                              const float* gamma, const float* partials,
                              const float* count_ptr, float* dx, long n, int h,
                              bool relu, float keep_inv, hipStream_t s);
void launch_bn_bwd_apply_only16(const void* g, const void* x, const void* y,
                                const float* mean, const float* invstd,
                                const float* gamma, const float* partials,
                                const float* count_ptr, void* dx, long n,
                                int h, bool relu, float keep_inv,
                                const unsigned char* mask, hipStream_t s);

void launch_quantile_loss_fwd(const float* y, const float* y_hat, float* out,
                              long b, float tau, hipStream_t s);
void launch_quantile_loss_bwd(const float* g, const float* y,
                              const float* y_hat, float* dy_hat, long b,
                              float tau, hipStream_t s);
void launch_eval_metrics(const float* y, const float* y_hat, float* out3,
                         long b, float tau, hipStream_t s);
void launch_adam(float* p, const float* g, float* m, float* v, float* state,
                 long numel, float lr, float b1, float b2, float eps,
                 float gscale, hipStream_t s);
void launch_adam_dynamic(float* p, const float* g, float* m, float* v,
                         float* state, float* sstate, long numel, float lr,
                         float b1, float b2, float eps, float backoff,
                         float growth, float interval, hipStream_t s);
void launch_adam_ex(float* p, const float* g, float* m, float* v,
                    float* state, float* sstate, float* hstate, float* slab,
                    int slab_len, const unsigned char* decay_mask,
                    const float* lr_table, long table_len, long numel,
                    float lr, float b1, float b2, float eps, float gscale,
                    float wd, float max_norm, float backoff, float growth,
                    float interval, hipStream_t s);

// ---- gemm.hip -------------------------------------------------------------
// NT: c[m, n] = a[m, k] . b[n, k]^T + bias; NN: c[m, k2] = a[m, n] . b[n, k2];
// TN: c[n, k2] = a[m, n]^T . b[m, k2], dbias[n] = column sums of a (or null)
void launch_gemm_f32_nt(const float* a, const float* b, const float* bias,
                        float* c, int m, int n, int k, bool relu,
                        hipStream_t s);
void launch_gemm_f32_nn(const float* a, const float* b, const float* bias,
                        float* c, int m, int n, int k2, bool relu,
                        hipStream_t s);
void launch_gemm_f32_tn(const float* a, const float* b, float* c, float* dbias,
                        int m, int n, int k2, hipStream_t s);
void launch_colsum(const float* g, float* out, long m, int n, hipStream_t s);
void launch_embed_fold_gemm(const float* G, const float* w, float* out,
                            int rows, int K, int h, int ldw, int col0,
                            bool accumulate, hipStream_t s);

// ---- gemm_bf16.hip --------------------------------------------------------
// fp32 in and out, bf16 / fp16 operands in the matrix cores
void launch_gemm_bf16_nt(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k, bool relu,
                         hipStream_t s);
void launch_gemm_bf16_nn(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k2, bool relu,
                         hipStream_t s);
void launch_gemm_bf16_tn(const float* a, const float* b, float* c,
                         float* dbias, int m, int n, int k2, hipStream_t s);
void launch_gemm_fp16_nt(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k, bool relu,
                         hipStream_t s);
void launch_gemm_fp16_nn(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k2, bool relu,
                         hipStream_t s);
void launch_gemm_fp16_tn(const float* a, const float* b, float* c,
                         float* dbias, int m, int n, int k2, hipStream_t s);
// o16: fp32 x and w, bf16 y and g
void launch_gemm_bf16_nt_o16(const float* a, const float* b, const float* bias,
                             void* c, int m, int n, int k, hipStream_t s);
void launch_gemm_bf16_nn_a16(const void* a, const float* b, float* c, int m,
                             int n, int k2, hipStream_t s);
void launch_gemm_bf16_tn_a16(const void* a, const float* b, float* c,
                             float* dbias, int m, int n, int k2,
                             hipStream_t s, bool acc = false);
void launch_gemm_skinny_nn(const void* g, const float* w, float* dx, int m,
                           int n, int k2, hipStream_t s);
// a16: bf16 x, y and g; bf16 or fp16 compute
void launch_gemm_bf16_nt_a16o16(const void* a, const float* b,
                                const float* bias, void* c, int m, int n,
                                int k, hipStream_t s);
void launch_gemm_bf16_nn_a16o16(const void* a, const float* b, void* c, int m,
                                int n, int k2, hipStream_t s);
void launch_gemm_bf16_tn_a16b16(const void* a, const void* b, float* c,
                                float* dbias, int m, int n, int k2,
                                hipStream_t s, bool acc = false);
void launch_gemm_fp16_nt_a16o16(const void* a, const float* b,
                                const float* bias, void* c, int m, int n,
                                int k, hipStream_t s);
void launch_gemm_fp16_nn_a16o16(const void* a, const float* b, void* c, int m,
                                int n, int k2, hipStream_t s);
void launch_gemm_fp16_tn_a16b16(const void* a, const void* b, float* c,
                                float* dbias, int m, int n, int k2,
                                hipStream_t s, bool acc = false);
// glds (direct-to-LDS staging) kernels over bf16 weight images
void launch_convert_w16(const float* w, void* o, long numel, hipStream_t s);
void launch_convert_w16_both(const float* w, void* o, void* ot, int rows,
                             int cols, hipStream_t s);
void launch_transpose_convert_w16(const float* w, void* o, int rows, int cols,
                                  hipStream_t s);
void launch_gemm_a16_glds_nt(const void* a, const void* b16, const float* bias,
                             void* c, int c16, int m, int n, int k, bool relu,
                             hipStream_t s);
void launch_gemm_a16_resident_nt(const void* a, const void* b16,
                                 const float* bias, void* c, int m, int n,
                                 int k, hipStream_t s);
// the forward kernel (gemm_dispatch::FwdVariant) a shape takes in this
// process, and the test hook that overrides it
int fwd_variant_for(int m, int n, int k);
void set_fwd_variant_hook(int v);
void launch_gemm_a16_glds_tn(const void* a, const void* b, float* c,
                             float* dbias, int m, int n, int k2,
                             hipStream_t s, bool acc = false, int tile = 0);
// the tile (gemm_dispatch::TnTile) that launcher runs for a shape it
// supports: `tile` if forced (-1 where the shape does not allow it), else
// the process-wide override (set_glds_tn_tile) or the dispatch's choice
int glds_tn_tile_for(int m, int n, int k2, int tile);
void set_glds_tn_tile(int tile);
// grouped P-table GEMMs (all layers, both tables, one launch each)
int ptables_max_groups();
void launch_ptables_fwd(int groups, const float* const* a,
                        const float* const* w, void* const* c, const int* m,
                        int n, int k, hipStream_t s);
void launch_ptables_dgrad(const void* const* dp, const float* const* w,
                          const int* npairs, float* const* out, const int* m,
                          int h, int splits, const bool* addto,
                          hipStream_t s);
bool launch_ptables_wgrad(int groups, const void* const* dp,
                          const float* const* a, float* const* dw,
                          const int* m, int h, bool probe, hipStream_t s,
                          const bool* sink = nullptr);
