// Every host entry point of se3_transformer_amd._C, declared once. Each
// .hip file that defines one includes this header; bindings.cpp binds them.
#pragma once

#include <torch/extension.h>

using torch::Tensor;

// pairconv.hip, pairconv_bwd.hip, pack_w.hip. Any mo, miF >= 1: mo_ of the
// four kernels is the padded ceil8(mo) and U, G, the packs and du's bias carry
// zero pads (pairconv_common.h); out (E, mo, O) and a 3-D dW (mo, miF, 128)
// name the true sizes. pack_w_both takes the true mo and pads.
int64_t pairconv_opad(int64_t O);
void pairconv_fwd_opad(Tensor H, Tensor W, Tensor Ut, Tensor out, int64_t mo_);
void pairconv_bwd_dh(Tensor G, Tensor U, Tensor Wt, Tensor dH, int64_t mo_, int64_t O_);
void pairconv_bwd_dw(Tensor G, Tensor U, Tensor Ht, Tensor dW, Tensor db, int64_t mo_,
                     int64_t O_);
void pairconv_bwd_du(Tensor H, Tensor W, Tensor bias, Tensor G, Tensor dU,
                     int64_t mo_, int64_t O_);
void pack_w_both(Tensor W, Tensor Pf, Tensor Pdh, int64_t mo_);
void pack_g(Tensor grad, Tensor G);
// radial.hip
void radial_trunk_fwd(Tensor X, Tensor W0, Tensor p0, Tensor W3, Tensor p3, Tensor H,
                      Tensor yh0, Tensor yh3, Tensor rs01, double eps);
void radial_trunk_bwd(Tensor dH, Tensor X, Tensor W0, Tensor p0, Tensor W3, Tensor W3t,
                      Tensor p3, Tensor yh0, Tensor yh3, Tensor rs01, Tensor dW0,
                      Tensor dp0, Tensor dW3, Tensor dp3, Tensor dX, double eps);
// ubuild.hip
void ubuild_fwd(Tensor B, Tensor X, Tensor U, int64_t O, int64_t I, int64_t F);
void ubuild_bwd_dx(Tensor B, Tensor dU, Tensor dX, int64_t O, int64_t I, int64_t F);
void ubuild_bwd_db(Tensor X, Tensor dU, Tensor dB, int64_t O, int64_t I, int64_t F);
void ubuild_gather_fwd(Tensor B, Tensor Xn, Tensor rows, Tensor U, int64_t O, int64_t I,
                       int64_t F);
void ubuild_gather_bwd_dx(Tensor B, Tensor dU, Tensor rows, Tensor dXn, int64_t O,
                          int64_t I, int64_t F);
void ubuild_gather_bwd_db(Tensor Xn, Tensor rows, Tensor dU, Tensor dB, int64_t O,
                          int64_t I, int64_t F);
// sh_basis.hip
void sh_basis_fwd(Tensor rel, Tensor qcat, Tensor normtab, Tensor meta, Tensor out,
                  int64_t L);
void sh_basis_bwd(Tensor rel, Tensor qcat, Tensor normtab, Tensor meta, Tensor dK,
                  Tensor drel, int64_t L);
// knn.hip
void knn_graph(Tensor coors, Tensor nmask, Tensor allow, Tensor sparse, Tensor idx,
               Tensor dist, Tensor rel, Tensor m, int64_t k, double radius, bool causal);
int64_t knn_max_lds_bytes();
// attn2.hip
void attn2_fwd(Tensor q, Tensor k, Tensor v, Tensor mask, Tensor qf, Tensor kf,
               Tensor out, Tensor lse, int64_t n, int64_t heads, double scale,
               bool kv_one, int64_t jr, int64_t rot);
void attn2_bwd(Tensor q, Tensor k, Tensor v, Tensor mask, Tensor qf, Tensor kf,
               Tensor out, Tensor lse, Tensor g, Tensor dq, Tensor dk, Tensor dv,
               int64_t n, int64_t heads, double scale, bool kv_one, int64_t jr,
               int64_t rot);
// norm_se3.hip
void norm_se3_nl_fwd(Tensor t, Tensor scale, Tensor out, double eps, int64_t nonlin);
void norm_se3_nl_bwd(Tensor t, Tensor scale, Tensor dout, Tensor dt, Tensor dscale,
                     double eps, int64_t nonlin);
int64_t norm_se3_gated_max_c();
void norm_se3_gated_fwd(Tensor t, Tensor W, Tensor out, Tensor gate, double eps,
                        int64_t nonlin);
void norm_se3_gated_bwd(Tensor t, Tensor Wt, Tensor gate, Tensor dout, Tensor dt,
                        Tensor dgate, Tensor nu, double eps, int64_t nonlin);
// egnn.hip
void egnn_rel_dist_fwd(Tensor ht, Tensor idx, Tensor dist);
void egnn_rel_dist_bwd(Tensor ht, Tensor idx, Tensor gdist, Tensor dht);
void egnn_htype_update_fwd(Tensor ht, Tensor idx, Tensor w, Tensor sc, Tensor bi,
                           Tensor upd, double eps);
void egnn_htype_update_bwd(Tensor ht, Tensor idx, Tensor w, Tensor sc, Tensor bi,
                           Tensor g, Tensor dht, Tensor dw, Tensor dsc, Tensor dbi,
                           double eps);
