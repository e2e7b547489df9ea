// backward_layout.h — flat parameter layout (Dynamics.parameters() order) shared by the EGNN backward kernels
// (egnn_backward.hip: fully-connected graph, egnn_backward_sparse.hip: pocket radius graph).
#pragma once
#include "pack_layout.h"

namespace {

constexpr int H = 128;                         // hidden_nf
constexpr int MAX_FIN = 64;                    // node input width of the embedding (nf + time + context)

struct Offs {                                  // parameter offsets (floats) of one network
    long emb_w, emb_b, out_w, out_b;
    long blk0, blk_stride, gcl_stride, equiv;  // block k starts at blk0 + k * blk_stride, GCL s at + s * gcl_stride
};

// per GCL: edge_mlp.0 [H, 2H+2] + b, edge_mlp.2 [H, H] + b, node_mlp.0 [H, 2H] + b, node_mlp.2 [H, H] + b
constexpr long G_E0W = 0, G_E0B = G_E0W + long(H) * (2 * H + 2), G_E2W = G_E0B + H, G_E2B = G_E2W + long(H) * H,
               G_N0W = G_E2B + H, G_N0B = G_N0W + long(H) * 2 * H, G_N2W = G_N0B + H, G_N2B = G_N2W + long(H) * H,
               G_SIZE = G_N2B + H;
// gcl_equiv.coord_mlp: 0 [H, 2H+2] + b, 2 [H, H] + b, 4 [1, H]
constexpr long C_0W = 0, C_0B = C_0W + long(H) * (2 * H + 2), C_2W = C_0B + H, C_2B = C_2W + long(H) * H,
               C_4W = C_2B + H, C_SIZE = C_4W + H;

__host__ __device__ inline Offs param_offsets(int fin, int sub) {
    Offs o;
    o.emb_w = 0;
    o.emb_b = o.emb_w + long(H) * fin;
    o.out_w = o.emb_b + H;
    o.out_b = o.out_w + long(fin) * H;
    o.blk0 = o.out_b + fin;
    o.gcl_stride = G_SIZE;
    o.equiv = G_SIZE * sub;
    o.blk_stride = o.equiv + C_SIZE;
    return o;
}

__host__ __device__ inline long param_count(int fin, int layers, int sub) {
    const Offs o = param_offsets(fin, sub);
    return o.blk0 + o.blk_stride * layers;
}

}  // namespace
