// What the ResNet backbone's forward (resnet.hip) hands its backward (resnet_bwd.hip): the net of a trainable forward as a table, one
// row per launch in launch order, with the place of every activation the backward reads.  Pure host.  resnet.hip defines train_net on
// top of its own plan, so the two units cannot disagree about a plane size, a producer or an offset.  Below it, on the device: the
// BatchNorm fold's scale and rounding rule, which resnet.hip, resnet_bwd.hip and resnet_repack.hip share.
#pragma once
#include <cstdint>

#include "sbev_common.hpp"

namespace sbev_resnet {

constexpr long long kNotKept = INT64_MIN;      // TLayer::act of a frozen layer whose output ping-pongs in the forward's workspace

struct TLayer {
    int kind;                   // 0 stem, 1 pool, 2 convolution
    int Cin, Cout, taps, stride, H, W, h, w;
    int in_layer, res_layer;    // producing launches (-1: the image / none)
    int stage;                  // 0-based stage of a block's convolution, -1 for the stem and the pool
    int block;                  // block inside the stage
    int which;                  // 0 conv1, 1 conv2, 2 downsample, 3 conv3
    int out_k;                  // k where this launch writes outs[k], else -1
    long long rows;             // n h w
    long long pack_off;         // byte offset of its image in the forward's pack
    long long act;              // byte offset of its output in the activation buffer; kNotKept; unused (0) where out_k >= 0
};

struct TrainNet {
    int n_layers, n_out, first_kept;      // first_kept: the launch whose output the first trainable block reads
    int first_trainable_stage;            // 1 ..
    TLayer layer[SBEV_RESNET_MAX_LAYERS];
    int out_layer[4];
    long long acts_bytes, ws_bytes, pack_bytes;
};

// sbev_resnet_plan's refusals under `who`, then first_trainable_stage in 1 .. num_stages
int train_net(const char* who, int depth, const int32_t* stage_blocks, int num_stages, int base, int64_t n, int H, int W, int n_out,
              const int32_t* out_indices, int first_trainable_stage, TrainNet* t);

// ---------------------------------------------------------------- the BatchNorm fold (device), stated once for the three units
// Their weight images must agree bit for bit (resnet.hip: sbev_resnet_pack_weights, resnet_bwd.hip: sbev_resnet_pack_weights_bwd,
// resnet_repack.hip: sbev_resnet_repack); all three are built with -ffp-contract=off, every operation is rounded on its own.

// s = gamma / sqrt(var + eps)
__device__ __forceinline__ float bn_fold_scale(float gamma, float var, float eps) { return gamma / sqrtf(var + eps); }

// w' = fp16(fp32(w s)): TWO roundings, the product to fp32 first, then to fp16.  The product exists as an fp32 value, rounded, before it
// is converted: without the register barrier the backend folds multiply and conversion into v_fma_mixlo_f16, ONE rounding -- other bits
// in 1 of ~10^4 elements.  bn_fold_round is the second rounding alone, of a product w * s the caller already holds: a kernel that
// gathers several elements per lane forms all its products first and rounds them afterwards, so that the barriers stand behind the
// loads and every gather stays in flight (a barrier between two gathers makes each wait for the one before).
__device__ __forceinline__ _Float16 bn_fold_round(float product) {
    asm volatile("" : "+v"(product));
    return (_Float16)product;
}

__device__ __forceinline__ _Float16 bn_fold_weight(float w, float s) { return bn_fold_round(w * s); }

}  // namespace sbev_resnet
