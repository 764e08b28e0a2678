// The encoder layer over an adjacency WITH VALUES — GraphConv / GCNConv(normalize=False) on an adj_t that carries one value per stored edge (the
// reference's gcn_normalization / adj_normalization and its real edge weights, Link_prediction_model/utils.py:93-106, trainer_link_prediction.py:276-342):
//     agg[v] = sum_{j in row v} w_csr[j] * h[col[j]]                                              (acc += w * x, edge by edge, fp32)
//     out[v] = epi( [agg[v] | self[v]] @ B + bias )
// k_sage_layer of cb_sage_core.h with its per-edge flag: the kernel, the image (cb_sage_image_f32), the epilogue, agg_out and the shape conditions
// (cb_sage_layer_supported) are cb_sage_layer_f32's; w_csr takes the place of the two scale vectors and is read by the lane that reads col[j], at the same
// absolute index, with the same streaming load — 4 bytes per edge next to a 1 KiB gathered row.  Hub rows are finished beforehand by the hub kernels
// with the same flag and read back from agg_out.  Bit for bit cb_spmm_csr_ew_f32 followed by cb_gemm_nn_f32 on the materialised [agg | self].
#include "cb_sage_core.h"

using namespace cb;

extern "C" int cb_ewlayer_f32(const cb_csr_view* g, const float* w_csr, const float* h, int64_t ld_h, const float* self, int64_t ld_self, const void* image,
                              const float* bias, int relu, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, float* agg_out,
                              int64_t ld_agg, int32_t agg_hubs_only, float* out, int64_t ld_out, void* stream) {
  return sage_layer_launch<true>("cb_ewlayer_f32", g, h, ld_h, self, ld_self, nullptr, nullptr, w_csr, image, bias, relu, drop_p, seed, seed_dev, row0, agg_out,
                                 ld_agg, agg_hubs_only, out, ld_out, stream);
}
