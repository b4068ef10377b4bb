// Row chains of the decoder layer: every op between the big mixing GEMMs and the self attention is ROW-LOCAL (a Linear, a
// LayerNorm, a ReLU, refine_bbox, the sample points and their projection: query i's output depends on query i only), so a
// workgroup that owns R = 4 queries runs the whole chain with the activations in LDS instead of one full-chip launch per op
// (sparsebev_transformer.py:166-183 are 14 such ops per layer; the per-op launches cost 5-10 us each for < 1 us of arithmetic).
//   TAIL (+ FRONT of the next layer): split-K slabs of mixing.out_proj -> + bias + residual -> norm2 -> ffn -> norm3 ->
//       cls_branch / reg_branch -> refine_bbox  [-> position_encoder -> x = feat + pos -> attention in-projection]
//   ATT: attention out-projection + residual -> norm1 -> sampling_offset / scale_weights Linear -> sample points ->
//       projection into the T*6 cameras, first-hit selection, level softmax (sample_point.hpp)
//   FRONT: position_encoder + in-projection of layer 0
//
// GEMM engine (M = 4 rows, so neither a 16- nor a 32-row MFMA tile fits): v_mfma_f32_4x4x1_16b_f32 with the A-matrix
// BROADCAST modifier (cbsz = 4, abid = k): the 16 blocks of the instruction are 16 groups of 4 output COLUMNS (lane = one
// of 64 columns), all multiplied by the same 4 rows of block `abid` of the A register -- A holds 16 k-values x 4 rows (one
// ds_read_b32 per 16 k), B is the lane's own weight column, D is 4 rows x 64 columns in 4 VGPRs.  Exact fp32 (fmaf chain)
// at the full f32 MFMA rate (8.6-9.8 cycles per instruction measured), no operand duplication.  The weights are streamed
// from L2 (every workgroup reads every weight: that stream, ~50 B/clk/CU through global_load_lds_dwordx4, is the bound), so
// they are PRE-PACKED (sbev_decoder_chain_pack) in the order the lanes consume them: a wave-load is 1 KB of contiguous memory.
// Work split: 8 waves; a unit (one or two independent Linears reading LDS rows) is cut into items of 64 columns x 128 k;
// item i goes to wave i % 8 in round i / 8 and leaves its partial sums in LDS slot i; the unit's epilogue (wave = row)
// adds the k-halves in a fixed order, + bias, ReLU / residual / LayerNorm, and writes the next unit's input rows.
// Results equal the op-by-op launches to fp32 round-off (other summation order), not bit for bit; DESIGN_HISTORY.md section 4.
//
// In this file: the kernels (row_chain_kernel<PRE, RG, PAIR> in 11 instantiations and row_chain_fixed_kernel, the same body with a unit
// table compiled in, in 4; pack_kernel, copy_pad_kernel), the constexpr planner of the unit tables between them, then the host side,
// each thing described once: the table of the image's 12 matrices (kMats -> pack_map, the pack jobs, the warm spans), the table of the
// instantiations (kInst -> launch, the LDS attribute, chain_lds_ready), and the plan of a launch (chain_plan: instantiation, grid, both
// pair members' unit tables from ONE function of the share, warm span, small-vector range; pure host, exported as
// sbev_decoder_chain_plan).  launch_chain_front / _attn / _tail make the plan, bind the image and the activations, launch.  The sticky
// fault word the pair hand-off reports into lives in fault_word.hip; this file keeps its __device__ end (chain_pair_install).
#include "sbev_common.hpp"
#include "sample_point.hpp"
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

namespace {

constexpr int NWAVE = 8;
constexpr int DM = 256, FF = 512;    // embed_dims, ffn width (host-checked)
constexpr int LDX = DM + 8;          // LDS row strides: == 8 (mod 32) so the A read (4 rows x 16 k per 32 lanes) is conflict-free
constexpr int LDH = FF + 8;
static_assert(2 * LDX >= LDH, "branch rows alias the ffn hidden rows");

// The small vectors (biases, LayerNorm weights, the 3 -> 256 position-encoder weight) live behind the packed matrices in the
// chain_pack image, grouped per chain, and are copied into LDS at kernel start (one contiguous copy; every epilogue would
// otherwise pay a cold global load).  Float offsets inside the LDS parameter block:
constexpr int PV_OP_B = 0, PV_N2G = 256, PV_N2B = 512, PV_FFN0_B = 768, PV_FFN1_B = 1280, PV_N3G = 1536, PV_N3B = 1792,
              PV_CLS0_B = 2048, PV_CLS1G = 2304, PV_CLS1B = 2560, PV_CLS3_B = 2816, PV_CLS4G = 3072, PV_CLS4B = 3328,
              PV_CLS6_B = 3584, PV_REG0_B = 3648, PV_REG2_B = 3904, PV_REG4_B = 4160, PV_TAIL_END = 4224;
constexpr int PV_PE0_W = PV_TAIL_END, PV_PE0_B = PV_PE0_W + 768, PV_PE1G = PV_PE0_B + 256, PV_PE1B = PV_PE1G + 256,
              PV_PE3_B = PV_PE1B + 256, PV_PE4G = PV_PE3_B + 256, PV_PE4B = PV_PE4G + 256, PV_QKV_B = PV_PE4B + 256, PV_QKV_PAD = 832,
              PV_FRONT_END = PV_QKV_B + PV_QKV_PAD;
// attention chain (its own launch: offsets from the block start again)
constexpr int PV_AOUT_B = 0, PV_N1G = 256, PV_N1B = 512, PV_SAMP_B = 768, PV_ATTN_END = 1024;
constexpr int PV_IMAGE_FLOATS = PV_FRONT_END + PV_ATTN_END;      // in the image: [tail | front | attention]

enum Epi { EPI_FFN0, EPI_FFN1, EPI_BR1, EPI_BR2, EPI_OUT, EPI_PE3, EPI_QKV, EPI_AOUT, EPI_SAMP };
enum Pre { PRE_SLABS, PRE_FRONT, PRE_ATT };

struct Lin {
    const float* wp;     // packed weights of this Linear
    int in_off, ld;      // LDS rows it reads
    int KH;              // k-pieces per column group (RG = 1: K / 128)
    int items;           // 64-column groups x KH
    int chunks;          // 16-k chunks per item = K / (16 KHT); a multiple of 4
    int kh0, KHT;        // this Linear covers the k-pieces [kh0, kh0 + KH) of the KHT pieces of a full row (KHT == KH, kh0 == 0 but for
                         // the k-half a pair member takes of ffn.layers.1)
};
struct Unit {
    Lin a, b;            // b.items == 0: one Linear
    int epi;
    int col0;            // EPI_QKV: first output column of this unit
};

#ifdef SBEV_CHAIN_TRACE
#define SBEV_TRACE(i) if ((blockIdx.x == 7 || blockIdx.x == 15) && lane == 0) a.trace[(blockIdx.x == 15 ? 64 * 512 : 0) + wave * 64 + (i)] = (long long)__builtin_amdgcn_s_memrealtime();   // 100 MHz
#else
#define SBEV_TRACE(i)
#endif

// The kernel arguments: what every row-chain kernel takes (ChainCommon), behind either the unit tables (ChainArgs: row_chain_kernel,
// which reads them at run time) or the image's base alone (ChainArgsFx: row_chain_fixed_kernel, whose tables are constants of the
// instantiation, see "fixed plans" below).
struct UnitTab {
    Unit units[8];
    Unit units_b[8];             // pair mode: the second member's units (same count, same epilogues)
};
struct ChainCommon {
#ifdef SBEV_CHAIN_TRACE
    long long* trace;
#endif
    int n_units, pre, front;     // n_units: of the tables (a fixed kernel knows its own); front: EPI_OUT continues with the next layer's position encoder
    int n_pairs;                 // pair mode: pairs of workgroups (= row blocks)
    float* pair_x;               // pair mode: exchange rows [n_pairs][3][R][256] (ffn.1 partial sums of member 0 / 1, x rows)
    unsigned* pair_sync;         // pair mode: one arrival counter per pair; the ATTENTION chain of the same layer zeroes them:
    unsigned* zero_words; int n_zero;
    int debug_drop;              // test hook (sbev_debug_chain_pair_drop): member 1 of pair 0 leaves at once -- its partner must time out, not hang
    const float* warm;           // the launch's packed weights: one contiguous span of the chain_pack image ...
    int warm_lines;              // ... of this many 128-byte lines (L2 warm-up, see warm_l2)
    const float* vec;            // the launch's small vectors in the image -> LDS parameter block [vec_off, vec_off + vec_n)
    int vec_off, vec_n;
    long long M;                 // rows (B * Q)
    int Q;
    const float* slabs; int splits;      // PRE_SLABS: [splits, M, 256]
    const float* x1;             // [M, 256] residual of mixing.out_proj
    float* x3;                   // [M, 256] the layer's output rows
    const float* bbox;           // [M, 10] this layer's query boxes
    const float* vel_div;        // [B] or null
    float* cls_out;              // [M, num_classes]
    float* box_out;              // [M, 10]
    int num_classes;
    const float* feat;           // PRE_FRONT: [M, 256] query_feat
    float* x;                    // [M, 256]
    float* qkvt; int attn_in_rows;
    const float* att;            // PRE_ATT: [M, 256]
    float* x1_out;               // [M, 256]
    unsigned short* x1_frag;     // fp16 GEMM modes: x1 also as the generator's operand -- scaled fp16 hi | lo images in MFMA fragment order
    const float* x1_scale;       //   (gemm_bf16s.hip: [M/32][16 k-steps][2][64 lanes][8]), scaled by x1_scale[0] = 2^e; null otherwise
    float* so; int soN;          // so: null when the sample points are projected in here (proj.loc_bp set)
    sbev_ops::SamplePointArgs proj;
    float eps;
    uint32_t* skip_hdr;          // PRE_FRONT of a step with a prefix cache (sbev_common.hpp: prefix_clean), else null; read by that instantiation only
};
struct ChainArgs : UnitTab, ChainCommon {};
struct ChainArgsFx : ChainCommon {
    const float* image;          // the chain_pack image: the constant tables hold float offsets into it
};

// ---- the weight stream --------------------------------------------------------------------------------------------------
// A wave's items (in program order) form one stream of 4 KB chunks (64 columns x 16 k, 4 wave-loads of 1 KB).  The chunks
// go global -> LDS directly (global_load_lds_dwordx4) into a private 3-slot ring per wave; a chunk is read into registers
// and its slot refilled at once, so THREE chunks (12 KB per wave, 96 KB per CU) are in flight while one multiplies, also
// across item / unit boundaries (weights do not depend on activations).  The loads are issued
// and waited for by hand (inline asm, counted s_waitcnt vmcnt): hipcc waits vmcnt(0) before every LDS read that follows a
// compiler-visible LDS-DMA load, which would serialise the stream.  Vector-memory loads return in order, so "at most 4
// outstanding" means everything older than the newest chunk has landed; compiler-issued loads / stores in between only
// make these waits (and the compiler's own) more conservative.
constexpr int RING_SLOTS = 3;
constexpr int CHUNK_FLOATS = 1024;

// Rows per workgroup: R = 4 RG, RG = 1, 2 or 4 row groups of the 4-row MFMA (template parameter of the kernels).
//   RG = 1 (<= 1024 rows, round 2): the LDS-DMA ring above, items of 64 columns x 128 k, 16 partial-sum slots.
//   RG = 2 / 4 (round 3: up to 2048 / 4096 rows in ONE round of workgroups -- the batch configs, 3200 and 3600 rows, and the
//     1600-query config): every weight chunk multiplies RG row groups (RG x the MFMAs per byte streamed: at RG = 4 the launch
//     is as much MFMA- as stream-bound), so the LDS goes to the rows, the chunks travel global -> VGPR (a ring of 4 chunks =
//     64 registers, waits counted by the compiler), and a wave keeps a column group's k-pieces in its accumulators: items are
//     64 columns x (K / KH) k with KH chosen by pieces() so that a unit has ~8 items (<= 12 partial-sum slots).
// LDS map (float offsets):
template <int RG>
struct Lay {
    static constexpr int R = 4 * RG;
    static constexpr bool WIDE = RG > 1;
    static constexpr int MAX_SLOTS = WIDE ? 12 : 16;
    static constexpr int OFF_X2 = 0;                    // x2 (norm2 output) / x (attention input rows) / att rows
    static constexpr int OFF_X3 = OFF_X2 + R * LDX;     // x3 = the layer's output rows (next layer's query_feat) / x1
    static constexpr int OFF_H = OFF_X3 + R * LDX;      // ffn hidden rows; dead after ffn.layers.1, then:
    static constexpr int OFF_C = OFF_H;                 //   classification-branch rows / position-encoder rows
    static constexpr int OFF_R = OFF_H + R * LDX;       //   regression-branch rows
    static constexpr int OFF_P = OFF_H + 2 * R * LDX;   // partial sums [MAX_SLOTS][R][64]     (2 R LDX >= R LDH)
    static constexpr int LDS_FLOATS = OFF_P + MAX_SLOTS * R * 64;
    static constexpr int OFF_RING = LDS_FLOATS;                                                      // [NWAVE][RING_SLOTS][CHUNK_FLOATS]
    static constexpr int OFF_DUMP = OFF_RING + (WIDE ? 0 : NWAVE * RING_SLOTS * CHUNK_FLOATS);     // [NWAVE][64] sink of the warm-up loads
    static constexpr int OFF_PARAM = OFF_DUMP + NWAVE * 64;                                          // the launch's small vectors (PV_* offsets)
    static constexpr int LDS_TOTAL_FLOATS = OFF_PARAM + PV_FRONT_END;
    static constexpr int RPW = (R + NWAVE - 1) / NWAVE;                                              // input rows per wave in the prologue
    static_assert(LDS_TOTAL_FLOATS * 4 <= 160 * 1024, "LDS budget of one CU");
};
struct Offs { int x2, x3, h, c, r; };        // the same offsets for the host-side unit tables
template <int RG> constexpr Offs offs_of() { return Offs{Lay<RG>::OFF_X2, Lay<RG>::OFF_X3, Lay<RG>::OFF_H, Lay<RG>::OFF_C, Lay<RG>::OFF_R}; }

// L2 warm-up.  The L2 is cold for the weights at every launch (a whole layer of GEMM / gather traffic went through it), and
// the workgroups of an XCD stream the same lines in near lock-step, so each line's HBM / Infinity-Cache miss latency would be
// seen by all of them, every round.  Instead the workgroups of an XCD (workgroup i runs on XCD i % 8) split the launch's
// weight span between them and touch one dword per 128-byte line of their slice up front, while the prologue runs; the
// loads go to an LDS sink (no register to keep alive) and are older than every chunk load, so the counted waits stay valid.
template <int RG>
__device__ __forceinline__ void warm_l2(const ChainCommon& a, int wave, int lane) {
    const int per_xcd = ((int)gridDim.x + 7) / 8;
    const int parts = per_xcd < 32 ? per_xcd : 32;
    const int part = ((int)blockIdx.x / 8) % parts;
    const int n = (a.warm_lines + parts - 1) / parts;
    const int l0 = part * n;
    const int l1 = min(a.warm_lines, l0 + n);
    const unsigned dump = (unsigned)(Lay<RG>::OFF_DUMP + wave * 64) * 4u;
    for (int l = l0 + wave * 64; l < l1; l += NWAVE * 64) {
        const int line = min(l + lane, l1 - 1);
        const unsigned voff = (unsigned)line * 128u;
        asm volatile(
            "s_mov_b32 m0, %0\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dword %1, %2\n\t"
            :
            : "s"(dump), "v"(voff), "s"(a.warm)
            : "memory");
    }
}

struct Walk {            // position of a wave in its item stream
    int u, it, step;
};

__device__ __forceinline__ const float* lin_item_weights(const Lin& l, int j) {
    const int piece = l.KHT == l.KH ? j : (j / l.KH) * l.KHT + l.kh0 + j % l.KH;
    return l.wp + (long long)piece * (l.chunks * CHUNK_FLOATS);
}
__device__ __forceinline__ const float* item_weights(const Unit& un, int it) {
    const bool second = it >= un.a.items;
    return lin_item_weights(second ? un.b : un.a, it - (second ? un.a.items : 0));
}

// (M0 carries the LDS destination of an LDS-DMA load and is written inside the asm block; hipcc does not use M0 anywhere else
// in these kernels -- LDS instructions need no M0 on gfx9+, there is no dynamic register indexing -- checked in the ISA.)
__device__ __forceinline__ void issue_chunk(const float* g, unsigned lds_byte, unsigned voff) {
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
        :
        : "s"(lds_byte), "v"(voff), "s"(g)
        : "memory");
}

struct Stream {
    Walk iw;             // item of the next chunk to issue
    const float* g;      // its weights (next chunk)
    int nchunk;          // chunks of that item
    int issued, used;    // chunk counters
    int islot, uslot;    // issued % RING_SLOTS, used % RING_SLOTS
    unsigned ring_byte;  // LDS byte address of this wave's ring
    unsigned voff;       // lane * 16
    // fixed plans only (FxTab): the item being multiplied and the wave's next one -- their weights; whether there is a next one; whether
    // the stream has anything left to issue
    const float *g_cur, *g_next;
    bool has_next, live;
};

// RG > 1: the next chunk of the stream into 16 registers (four 1 KB wave-loads; the compiler counts the waits)
struct RChunk { float4 q[4]; };

// How the stream finds its way through a unit table (TAB).  RtTab walks the table in the kernel arguments: it carries a position (Walk)
// and seeks the next item whenever one is issued to its end.  FxTab ("fixed plans" below) knows the table at compile time and is told
// where the multiply is (begin_item, begin_round): what to issue follows from that with immediates.
struct RtTab {
    const ChainArgs& a;
    const Unit* U;       // the workgroup's unit table (kernel arguments)

    // first item of this wave at or after (u, it)
    __device__ __forceinline__ void settle(Walk& w, int wave) const {
        while (w.u < a.n_units && w.it >= U[w.u].a.items + U[w.u].b.items) {
            ++w.u;
            w.it = wave;
        }
    }
    __device__ __forceinline__ void seek(Stream& st, int wave) const {
        settle(st.iw, wave);
        st.iw.step = 0;
        if (st.iw.u < a.n_units) {
            const Unit& un = U[st.iw.u];
            st.g = item_weights(un, st.iw.it);
            st.nchunk = st.iw.it >= un.a.items ? un.b.chunks : un.a.chunks;
        }
    }
    __device__ __forceinline__ void issue(Stream& st, int wave) const {
        if (st.iw.u >= a.n_units) return;
        issue_chunk(st.g + st.iw.step * CHUNK_FLOATS, st.ring_byte + (unsigned)st.islot * (CHUNK_FLOATS * 4), st.voff);
        ++st.issued;
        st.islot = st.islot == RING_SLOTS - 1 ? 0 : st.islot + 1;
        if (++st.iw.step == st.nchunk) {
            st.iw.it += NWAVE;
            seek(st, wave);
        }
    }
    // The loads are UNCONDITIONAL (past the end of the stream a wave re-reads the first chunk of its last item, <= 16 KB per wave):
    // a load under a branch would make the number of younger loads unknown to the compiler, which then waits vmcnt(0) before every
    // chunk instead of vmcnt(12).
    __device__ __forceinline__ void load(Stream& st, int wave, int lane, RChunk& c) const {
        const float* g = st.g + st.iw.step * CHUNK_FLOATS + lane * 4;
#pragma unroll
        for (int m = 0; m < 4; ++m) c.q[m] = *reinterpret_cast<const float4*>(g + 256 * m);
        if (st.iw.u < a.n_units && ++st.iw.step == st.nchunk) {
            st.iw.it += NWAVE;
            seek(st, wave);
        }
    }
    template <class UC> __device__ __forceinline__ void begin_item(UC, Stream&, int, int) const {}
    __device__ __forceinline__ void begin_round(Stream&, int, int) const {}
};
constexpr int RDEPTH = 4;        // chunks in registers per wave (one multiplying, three on their way)

#define SBEV_MF(KK, BV) acc[(KK) & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(av, BV, acc[(KK) & 1], 4, KK, 0);
#define SBEV_MSTEP(m, q) SBEV_MF(4 * (m) + 0, q.x) SBEV_MF(4 * (m) + 1, q.y) SBEV_MF(4 * (m) + 2, q.z) SBEV_MF(4 * (m) + 3, q.w)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one item (64 columns x 128 k) of Linear `l`: 8 chunks from the ring; partial sums -> P[slot]
template <class TAB>
__device__ __forceinline__ void mma_item(const TAB& a, Stream& st, const Lin& l, int j, float* smem, int pslot, int lane, int wave) {
    constexpr int R = 4, OFF_RING = Lay<1>::OFF_RING, OFF_P = Lay<1>::OFF_P;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int kh = j % l.KH;
    const float* arow = smem + l.in_off + kh * 128 + (lane & 3) * l.ld + (lane >> 2);
    const float* ring = smem + OFF_RING + wave * (RING_SLOTS * CHUNK_FLOATS) + lane * 4;
    for (int s = 0; s < 8; ++s) {
        const int ahead = st.issued - st.used;             // chunks in flight incl. this one
        if (ahead >= 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (ahead == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float av = arow[s * 16];
        const float* slot = ring + st.uslot * CHUNK_FLOATS;
        const float4 q0 = *reinterpret_cast<const float4*>(slot);
        const float4 q1 = *reinterpret_cast<const float4*>(slot + 256);
        const float4 q2 = *reinterpret_cast<const float4*>(slot + 512);
        const float4 q3 = *reinterpret_cast<const float4*>(slot + 768);
        // the chunk is in registers: its slot is refilled right away (three chunks in flight while this one multiplies)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ++st.used;
        st.uslot = st.uslot == RING_SLOTS - 1 ? 0 : st.uslot + 1;
        a.issue(st, wave);
        __builtin_amdgcn_sched_barrier(0);
        SBEV_MSTEP(0, q0) SBEV_MSTEP(1, q1) SBEV_MSTEP(2, q2) SBEV_MSTEP(3, q3)
    }
    const f32x4 t = acc[0] + acc[1];
    float* p = smem + OFF_P + pslot * (R * 64) + lane;
    p[0] = t.x; p[64] = t.y; p[128] = t.z; p[192] = t.w;
}

// RG > 1: one item (64 columns x 16 l.chunks k) for the workgroup's RG row groups; the chunk registers rb[d] are consumed and
// refilled in ring order (l.chunks is a multiple of RDEPTH, so slot d of the ring is a compile-time register set)
template <int RG, class TAB>
__device__ __forceinline__ void mma_item_wide(const TAB& a, Stream& st, RChunk (&rb)[RDEPTH], const Lin& l, int j, float* smem, int pslot,
                                              int lane, int wave) {
    constexpr int NACC = RG >= 4 ? 1 : 2;          // >= 4 independent accumulator chains back to back
    f32x4 acc[RG][NACC];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[rg][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kh = l.kh0 + j % l.KH;
    const float* arow = smem + l.in_off + kh * (l.chunks * 16) + (lane & 3) * l.ld + (lane >> 2);
    float avn[RG];                                 // the A registers (16 k x 4 rows per row group) of the NEXT chunk: read one chunk ahead
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) avn[rg] = arow[rg * 4 * l.ld];
#pragma nounroll      // (a fixed plan's constant chunk count must not multiply the code: 64 RG MFMAs per round already)
    for (int s0 = 0; s0 < l.chunks; s0 += RDEPTH) {
        a.begin_round(st, l.chunks, s0);
#pragma unroll
        for (int d = 0; d < RDEPTH; ++d) {
            float av[RG];
            const int nxt = min(s0 + d + 1, l.chunks - 1);
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) { av[rg] = avn[rg]; avn[rg] = arow[nxt * 16 + rg * 4 * l.ld]; }
            __builtin_amdgcn_sched_barrier(0);
#define SBEV_MW(KK, BV)                                                                                                     \
    _Pragma("unroll") for (int rg = 0; rg < RG; ++rg)                                                                        \
        acc[rg][(KK) % NACC] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[rg], BV, acc[rg][(KK) % NACC], 4, KK, 0);
#define SBEV_MWSTEP(m, q) SBEV_MW(4 * (m) + 0, q.x) SBEV_MW(4 * (m) + 1, q.y) SBEV_MW(4 * (m) + 2, q.z) SBEV_MW(4 * (m) + 3, q.w)
            SBEV_MWSTEP(0, rb[d].q[0]) SBEV_MWSTEP(1, rb[d].q[1]) SBEV_MWSTEP(2, rb[d].q[2]) SBEV_MWSTEP(3, rb[d].q[3])
#undef SBEV_MWSTEP
#undef SBEV_MW
            __builtin_amdgcn_sched_barrier(0);
            a.load(st, wave, lane, rb[d]);               // refill: three chunks stay in flight while the next one multiplies
        }
    }
    float* p = smem + Lay<RG>::OFF_P + pslot * (Lay<RG>::R * 64) + lane;
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        f32x4 t = acc[rg][0];
        if (NACC == 2) t += acc[rg][NACC - 1];
        p[(rg * 4 + 0) * 64] = t.x; p[(rg * 4 + 1) * 64] = t.y; p[(rg * 4 + 2) * 64] = t.z; p[(rg * 4 + 3) * 64] = t.w;
    }
}

__device__ __forceinline__ float wsum(float v) { return sbev::wave_sum_dpp(v); }

// LayerNorm over 256 columns held as 4 per lane (column = lane + 64 c).  The weights are fetched (LDS) by LnW's constructor,
// i.e. where the caller declares it -- before the partial sums are gathered, so that their latency is not at the end of the chain.
struct LnW {
    float g[4], b[4];
    __device__ __forceinline__ LnW(const float* gp, const float* bp, int lane) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { g[c] = gp[lane + 64 * c]; b[c] = bp[lane + 64 * c]; }
    }
};
__device__ __forceinline__ void ln4(float (&v)[4], const LnW& w, float eps, bool relu) {
    const float mean = wsum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / DM);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) { const float d = v[c] - mean; q += d * d; }
    const float rstd = rsqrtf(wsum(q) * (1.f / DM) + eps);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float o = (v[c] - mean) * rstd * w.g[c] + w.b[c];
        v[c] = relu ? fmaxf(o, 0.f) : o;
    }
}

// partial sums of 4 column groups (cg0 .. cg0 + 3) of a Linear whose items start at slot `base`: k-halves added in order, + bias.
// KH is 2 (K = 256) or 4 (K = 512): specialised so that all LDS reads are in flight before the first add.
template <int KH, int R>
__device__ __forceinline__ void gather4_t(float (&v)[4], const float* P, int base, int cg0, int row, int lane, const float* bias, int bias0) {
    float t[4][KH];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) t[c][kh] = P[(base + (cg0 + c) * KH + kh) * (R * 64) + row * 64 + lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) s += t[c][kh];
        v[c] = s + bias[bias0 + lane + 64 * c];
    }
}
template <int R>
__device__ __forceinline__ void gather4(float (&v)[4], const float* P, int base, int KH, int cg0, int row, int lane, const float* bias,
                                        int bias0) {
    if (KH == 1) gather4_t<1, R>(v, P, base, cg0, row, lane, bias, bias0);
    else if (KH == 2) gather4_t<2, R>(v, P, base, cg0, row, lane, bias, bias0);
    else gather4_t<4, R>(v, P, base, cg0, row, lane, bias, bias0);
}

// the k-pieces of the 4 column groups of a Linear added in order, no bias (pair mode: a member's partial sums)
template <int R>
__device__ __forceinline__ void gather4_raw(float (&v)[4], const float* P, int KH, int row, int lane) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float s = 0.f;
        for (int kh = 0; kh < KH; ++kh) s += P[(c * KH + kh) * (R * 64) + row * 64 + lane];
        v[c] = s;
    }
}

// ---- pair mode: two workgroups share a row block (PAIR instantiations of the tail) --------------------------------------------------
// Every workgroup of a chain streams every weight, and a CU takes ~60 GB/s from the L2 whatever the row count (DESIGN_HISTORY.md
// section 10.3): the only way to stream less per CU is to split a row block's Linears between CUs.  A PAIR of workgroups owns R rows;
// both reduce the out-projection slabs and run norm2 (bit-identical x2 rows), then
//   ffn.layers.0    member s computes the hidden columns [256 s, 256 s + 256)            (its half of the weight's ROWS)
//   ffn.layers.1    member s sums over k in [256 s, 256 s + 256) -- the hidden columns it has -- for all 256 outputs; the partial
//                   sums are EXCHANGED, added member 0 + member 1 in both, + bias + residual -> norm3: x3 in both
//   branches        member 0 runs the classification branch, member 1 the regression branch, refine_bbox and (front) the position
//                   encoder; its x rows (feat + pos) are HANDED to member 0
//   in-projection   member 0 computes column groups 0 .. 7, member 1 the rest
// so a member streams ~1.65 of the 3.25 MB and the pair meets twice.  Hand-off (MI355X guide, inter-workgroup visibility): payload
// with 16-byte sc0 sc1 (write-through) stores, EVERY wave drains them, workgroup barrier, one lane adds to the pair's counter with a
// relaxed agent-scope atomic; the reader polls that word from one lane (s_sleep between polls; BOUNDED: a lost partner raises
// g_chain_pair_timeouts instead of hanging the GPU), workgroup barrier, sc0 sc1 loads.  Valid for any workgroup -> XCD placement; the
// block -> pair map puts both members on one XCD under round-robin dispatch (speed only).  The counters are zeroed by the attention
// chain of the same layer, which always runs between two tails on the stream (no memset node).
__device__ unsigned g_chain_pair_timeouts;
// ... and a STICKY fault word in pinned, device-mapped HOST memory (fault_word.hip installs the pointer through chain_pair_install, once per device): a
// timed-out hand-off also bumps it with a system-scope atomic, so the host sees the fault WITHOUT synchronising the device -- at the next
// sbev_decoder_forward / graph replay it is an error (SBEV_EFAULT), not eight silently wrong rows.  Read only on the timeout
// path: no kernel argument, no register in the hot loop.
__device__ unsigned* g_chain_pair_fault_host;
constexpr unsigned PAIR_POLL_LIMIT = 1u << 20;       // x (s_sleep 2 + one memory round trip, ~1 us): about a second

__device__ __forceinline__ void pair_store4(float* p, const float (&v)[4]) {
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(q) : "memory");
}
__device__ __forceinline__ void pair_load4(const float* p, float (&v)[4]) {
    f32x4 q;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(q) : "v"(p) : "memory");
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void pair_arrive(unsigned* word) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every wave: its payload stores have left
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pair_wait(unsigned* word, unsigned arrivals) {
    if (threadIdx.x == 0) {
        unsigned n = 0;
        while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < arrivals) {
            __builtin_amdgcn_s_sleep(2);
            if (++n > PAIR_POLL_LIMIT) {
                __hip_atomic_fetch_add(&g_chain_pair_timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                unsigned* const host_word = g_chain_pair_fault_host;
                if (host_word) __hip_atomic_fetch_add(host_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void store_rows(float* smem, int off, int ld, int row, int lane, const float (&v)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) smem[off + row * ld + lane + 64 * c] = v[c];
}

// position_encoder[0..2]: Linear(3 -> 256) + LayerNorm + ReLU of one row (sparsebev_transformer.py:116-119), into LDS
template <int RG>
__device__ __forceinline__ void pe0_row(const ChainCommon& a, float* smem, int row, int lane, float x0, float x1, float x2) {
    constexpr int OFF_PARAM = Lay<RG>::OFF_PARAM, OFF_C = Lay<RG>::OFF_C;
    const float* pv = smem + OFF_PARAM;
    const LnW lw(pv + PV_PE1G, pv + PV_PE1B, lane);
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = lane + 64 * c;
        const float* w = pv + PV_PE0_W + n * 3;
        v[c] = ((x0 * w[0] + x1 * w[1]) + x2 * w[2]) + pv[PV_PE0_B + n];
    }
    ln4(v, lw, a.eps, true);
    store_rows(smem, OFF_C, LDX, row, lane, v);
}

// ---- the plan of a launch, as far as it is a COMPILE-TIME function of the config: the image, the unit tables -----------------------------
// (constexpr: chain_plan evaluates it on the host at every launch, the fixed-plan kernels at compile time -- one description)
using Cfg = sbev_decoder_config;

// ---- the packed weight image, described once ------------------------------------------------------------------------------------------
// The 12 matrices in image order: the member of sbev_decoder_weights, its rows N and its columns K.  pack_map, the pack jobs,
// sbev_decoder_chain_pack_floats and the launches' warm spans ("matrices i .. j") all walk this one table.  Behind the matrices lie the
// small vectors [tail | front | attention] at their PV_* offsets (the vecs[] table of sbev_decoder_chain_pack).
enum Mat { M_FFN0, M_FFN1, M_CLS0, M_REG0, M_CLS3, M_REG2, M_CLS6, M_REG4, M_PE3, M_ATTN_IN, M_ATTN_OUT, M_SAMP, N_MAT };
constexpr int so_cols(const Cfg& c) { return c.G * c.P * (3 + c.L); }      // the sampling Linear's rows: 3 offsets + L level logits per point
constexpr int n_embed(const Cfg& c) { return c.D; }
constexpr int n_ffn(const Cfg& c) { return c.ffn; }
constexpr int n_cls(const Cfg& c) { return c.num_classes; }
constexpr int n_code(const Cfg& c) { return c.code_size; }
constexpr int n_qkv(const Cfg& c) { return c.attn_in_rows; }
struct MatDesc {
    const float* sbev_decoder_weights::*w;
    int (*N)(const Cfg&);
    int (*K)(const Cfg&);
};
constexpr MatDesc kMats[N_MAT] = {
    {&sbev_decoder_weights::ffn0_w, n_ffn, n_embed},      {&sbev_decoder_weights::ffn1_w, n_embed, n_ffn},
    {&sbev_decoder_weights::cls0_w, n_embed, n_embed},    {&sbev_decoder_weights::reg0_w, n_embed, n_embed},
    {&sbev_decoder_weights::cls3_w, n_embed, n_embed},    {&sbev_decoder_weights::reg2_w, n_embed, n_embed},
    {&sbev_decoder_weights::cls6_w, n_cls, n_embed},      {&sbev_decoder_weights::reg4_w, n_code, n_embed},
    {&sbev_decoder_weights::pe3_w, n_embed, n_embed},     {&sbev_decoder_weights::attn_in_w, n_qkv, n_embed},
    {&sbev_decoder_weights::attn_out_w, n_embed, n_embed}, {&sbev_decoder_weights::samp_w, so_cols, n_embed}};

constexpr long long packed_floats(int N, int K) { return (long long)((N + 63) / 64) * 64 * K; }

struct PackMap {     // float offsets into the chain_pack image: matrix i lies at [at[i], at[i + 1])
    long long at[N_MAT + 1];
    constexpr long long vec() const { return at[N_MAT]; }                      // the small vectors: [tail | front | attention], PV_* offsets
    constexpr long long total() const { return at[N_MAT] + PV_IMAGE_FLOATS; }
    constexpr int lines(int first, int last) const { return (int)((at[last + 1] - at[first]) / 32); }      // 128-byte lines of matrices first .. last
};
constexpr PackMap pack_map(const Cfg& c) {
    PackMap m{};
    for (int i = 0; i < N_MAT; ++i) m.at[i + 1] = m.at[i] + packed_floats(kMats[i].N(c), kMats[i].K(c));
    return m;
}

// Lin / Unit with the weights as a float offset into the image (-1: none) instead of a pointer
struct PLin { long long w; int in_off, ld, KH, items, chunks, kh0, KHT; };
struct PUnit { PLin a, b; int epi, col0; };
constexpr PLin kNone{-1, 0, LDX, 1, 0, 8, 0, 1};

// k-pieces per column group of a unit in which THIS SHARE of the row block (see Share) computes `cgs` column groups in all: RG = 1 keeps
// 128-k items; RG > 1 aims at 8 items per unit (one per wave; each piece at least 64 k = RDEPTH chunks)
// -- <= 12 slots; cost of a choice = sum over its rounds of (chunks per item) x (1 for a round of 5 .. 8 items: two waves per SIMD
// share the MFMA pipe; 1/2 for a last round of <= 4 items: waves 0 .. 3 sit on four different SIMDs)
// The two A/B switches of the environment that change a unit table.  They exist at run time only (chain_plan: env_tweaks); every fixed
// plan is built with kNoTweaks, so a launch under either switch finds no equal fixed table and takes the run-time-table kernel.
struct Tweaks {
    bool tie_large;      // SBEV_CHAIN_TIE_SMALL unset.  Equal cost: more, shorter items
    int q0_forced;       // SBEV_CHAIN_PAIR_Q0, -1 = unset: the in-projection's cut between the pair members
};
constexpr Tweaks kNoTweaks{true, -1};

constexpr int pieces(int rg, int cgs, int K, bool tie_large) {
    if (rg == 1) return 0;
    int best = 1;
    double best_cost = 1e30;
    for (int kh = 1; kh <= 4 && cgs * kh <= 12 && K / kh >= 16 * RDEPTH; kh *= 2) {
        const int items = cgs * kh, full = items / NWAVE, rest = items % NWAVE;
        const double cost = (K / (16.0 * kh)) * (full + (rest == 0 ? 0.0 : rest <= 4 ? 0.5 : 1.0));
        if (tie_large ? cost < best_cost + 1e-9 : cost < best_cost - 1e-9) { best_cost = cost; best = kh; }
    }
    return best;
}

constexpr Offs offs(int rg) { return rg == 1 ? offs_of<1>() : rg == 2 ? offs_of<2>() : offs_of<4>(); }

// Who computes a unit table: the one workgroup of a row block, or one member of the pair that shares it.
enum Share { WHOLE = -1, MEMBER0 = 0, MEMBER1 = 1 };

struct UnitTables {
    const Cfg& c;
    const PackMap& m;
    int rg;
    Offs o;
    Tweaks tw;

    constexpr int pieces(int rg_, int cgs, int K) const { return ::pieces(rg_, cgs, K, tw.tie_large); }

    // column groups [cg0, cg0 + ncg) of packed matrix `mat` as items of K / KH k each.  kh = 0: K / 128 (the RG = 1 items)
    constexpr PLin lin(int mat, int in_off, int ld, int kh = 0, int cg0 = 0, int ncg = -1) const {
        const int N = kMats[mat].N(c), K = kMats[mat].K(c);
        const int KH = kh > 0 ? kh : K / 128;
        if (ncg < 0) ncg = (N + 63) / 64 - cg0;
        return PLin{m.at[mat] + (long long)cg0 * K * 64, in_off, ld, KH, ncg * KH, K / (16 * KH), 0, KH};
    }
    // k-half `half` of packed matrix `mat` (pair mode): kh pieces of the half, i.e. pieces [half kh, half kh + kh) of 2 kh per row
    constexpr PLin lin_khalf(int mat, int in_off, int ld, int kh, int half) const {
        const int N = kMats[mat].N(c), K = kMats[mat].K(c);
        return PLin{m.at[mat], in_off, ld, kh, ((N + 63) / 64) * kh, K / (32 * kh), half * kh, 2 * kh};
    }

    // position encoder + attention in-projection (the front chain; the end of a tail with_front).  The position encoder runs where the
    // regression branch ran (WHOLE, MEMBER1).  In-projection column groups: WHOLE all of them, in units of at most 8; MEMBER1 those from
    // q0 onward -- it has the x rows in its LDS, member 0 gets them a hand-off (~1.5 us) later, so member 1 takes up to 8 column groups
    // (one round of 16-chunk items) and member 0 the rest (5 of config 2's 13: 10 items of 8 chunks) -- and MEMBER0 those below q0; a
    // member has exactly ONE in-projection unit, kNone where its share is empty.
    constexpr int front_units(PUnit* u, int n, Share sh) const {
        const int dcg = c.D / 64, qcg = (c.attn_in_rows + 63) / 64;
        u[n++] = PUnit{sh != MEMBER0 ? lin(M_PE3, o.c, LDX, pieces(rg, dcg, c.D)) : kNone, kNone, EPI_PE3, 0};
        const int q0_forced = tw.q0_forced;
        const int q0 = q0_forced >= 0 && q0_forced <= qcg ? q0_forced : (qcg > 8 ? qcg - 8 : qcg / 2);
        const int lo = sh == MEMBER1 ? q0 : 0, hi = sh == MEMBER0 ? q0 : qcg;
        const int cut = sh == WHOLE ? 8 : qcg + 1;
        if (sh != WHOLE && lo == hi) u[n++] = PUnit{kNone, kNone, EPI_QKV, lo * 64};
        for (int cg0 = lo; cg0 < hi; cg0 += cut) {
            const int n_here = hi - cg0 < cut ? hi - cg0 : cut;
            u[n++] = PUnit{lin(M_ATTN_IN, o.x2, LDX, pieces(rg, n_here, c.D), cg0, n_here), kNone, EPI_QKV, cg0 * 64};
        }
        return n;
    }

    // The tail's unit table, written once as a function of the share (see "pair mode" above the kernel):
    //   ffn.layers.0   WHOLE: all column groups; member s: half of them, from s x half on
    //   ffn.layers.1   WHOLE: all of k (lin); member s: k-half s (lin_khalf) for all columns
    //   branches       the classification side sits in Unit::a, the regression side in Unit::b; WHOLE carries both, MEMBER0 the
    //                  classification side, MEMBER1 the regression side (the other Lin is kNone)
    //   front          front_units
    // Every pieces() call gets the column groups THIS SHARE computes in that unit: both branch sides count for WHOLE (2 dcg; 2 for the
    // output unit), one side for a member (dcg; 1).  Both members get the same number of units and the same epilogue sequence.
    constexpr int tail_units(PUnit* u, Share sh, bool with_front) const {
        const int dcg = c.D / 64, fcg = c.ffn / 64;
        const bool cls = sh != MEMBER1, reg = sh != MEMBER0;
        const int sides = (cls ? 1 : 0) + (reg ? 1 : 0);
        const int f_ncg = sh == WHOLE ? fcg : fcg / 2, f_cg0 = sh == WHOLE ? 0 : sh * f_ncg;
        int n = 0;
        u[n++] = PUnit{lin(M_FFN0, o.x2, LDX, pieces(rg, f_ncg, c.D), f_cg0, f_ncg), kNone, EPI_FFN0, 0};
        u[n++] = PUnit{sh == WHOLE ? lin(M_FFN1, o.h, LDH, pieces(rg, dcg, c.ffn)) : lin_khalf(M_FFN1, o.h, LDH, pieces(rg, dcg, c.ffn / 2), sh),
                       kNone, EPI_FFN1, 0};
        const auto branch = [&](int mat_c, int in_c, int mat_r, int in_r, int cgs_side, int epi) {
            const int kh = pieces(rg, sides * cgs_side, c.D);
            return PUnit{cls ? lin(mat_c, in_c, LDX, kh) : kNone, reg ? lin(mat_r, in_r, LDX, kh) : kNone, epi, 0};
        };
        u[n++] = branch(M_CLS0, o.x3, M_REG0, o.x3, dcg, EPI_BR1);
        u[n++] = branch(M_CLS3, o.c, M_REG2, o.r, dcg, EPI_BR2);
        u[n++] = branch(M_CLS6, o.c, M_REG4, o.r, 1, EPI_OUT);
        return with_front ? front_units(u, n, sh) : n;
    }
};

// The unit tables of one launch: chain `pre` on row blocks of 4 rg rows, on pairs or not, the tail with or without the next front
struct PlanUnits {
    int n_units;
    PUnit units[2][8];           // [member]; units[1] in pair mode only (same count, same epilogues)
};
constexpr PlanUnits plan_units(const Cfg& c, int pre, int rg, bool pair, bool with_front, Tweaks tw) {
    const PackMap m = pack_map(c);
    const UnitTables t{c, m, rg, offs(rg), tw};
    PlanUnits p{};
    if (pre == PRE_FRONT) {
        p.n_units = t.front_units(p.units[0], 0, WHOLE);
    } else if (pre == PRE_ATT) {
        p.units[0][0] = PUnit{t.lin(M_ATTN_OUT, t.o.x2, LDX, t.pieces(rg, c.D / 64, c.D)), kNone, EPI_AOUT, 0};
        p.units[0][1] = PUnit{t.lin(M_SAMP, t.o.x3, LDX, t.pieces(rg, (so_cols(c) + 63) / 64, c.D)), kNone, EPI_SAMP, 0};
        p.n_units = 2;
    } else {
        p.n_units = t.tail_units(p.units[0], pair ? MEMBER0 : WHOLE, with_front);
        if (pair) (void)t.tail_units(p.units[1], MEMBER1, with_front);
    }
    return p;
}

// ---- fixed plans: unit tables as compile-time constants of a kernel instantiation ---------------------------------------------------------
// row_chain_supported fixes D, ffn and code_size, and num_classes <= 64 is one column group, so a launch's tables depend on nothing but
// this key.  The keys listed here get a kernel (row_chain_fixed_kernel) whose table is plan_units of the key, evaluated by the compiler:
// epilogue, item counts, LDS offsets and weight offsets are immediates, and the kernel arguments carry the image's base instead of 1.4 KB
// of tables.  A launch takes it when its own plan_units -- the same function, at run time -- gives the same words (fixed_match).
struct FixKey {
    int pre, rg, pair, with_front;
    int qcg, scg;                // 64-column groups of the attention in-projection and of the sampling Linear
};
constexpr int N_FIX = 4;         // config 2's launches: the tail on pairs with and without the next front, the attention chain, the front
constexpr FixKey fix_key(int i) {
    switch (i) {
    case 0: return FixKey{PRE_SLABS, 2, 1, 1, 13, 2};
    case 1: return FixKey{PRE_SLABS, 2, 1, 0, 13, 2};
    case 2: return FixKey{PRE_ATT, 1, 0, 0, 13, 2};
    default: return FixKey{PRE_FRONT, 1, 0, 0, 13, 2};
    }
}
constexpr bool same_key(const FixKey& a, const FixKey& b) {
    return a.pre == b.pre && a.rg == b.rg && a.pair == b.pair && a.with_front == b.with_front && a.qcg == b.qcg && a.scg == b.scg;
}
// a config with the key's column-group counts (any would do: the tables see a config through its column groups only)
constexpr Cfg key_cfg(const FixKey& k) {
    Cfg c{};
    c.D = DM; c.ffn = FF; c.code_size = 10; c.num_classes = 1;
    c.attn_in_rows = 64 * k.qcg;
    c.G = 1; c.P = 16 * k.scg; c.L = 1;       // G P (3 + L) = 64 scg sampling columns
    return c;
}
constexpr PlanUnits fixed_units(int i) {
    const FixKey k = fix_key(i);
    return plan_units(key_cfg(k), k.pre, k.rg, k.pair != 0, k.with_front != 0, kNoTweaks);
}

__host__ __device__ __forceinline__ Lin bound(const PLin& l, const float* pk) {
    return Lin{l.w < 0 ? nullptr : pk + l.w, l.in_off, l.ld, l.KH, l.items, l.chunks, l.kh0, l.KHT};
}

// The stream (see RtTab) over member MEM's table of fixed plan FIX.  A wave multiplies its items in a fixed order -- unit by unit, item
// wave, then wave + 8 -- and the stream runs a constant distance ahead of the multiply (RG = 1: 3 chunks through the LDS ring; RG > 1: the
// RDEPTH chunks in registers), less than the shortest item.  So what is issued belongs to the item being multiplied or to the wave's
// NEXT item, and begin_item -- called where the multiply enters item `it` of unit U, U a constant -- finds both with compares of
// `wave` and `it` against immediates; no table, no position to keep.
template <int FIX, int MEM>
struct FxTab {
    const float* image;
    static constexpr int N = fixed_units(FIX).n_units;
    template <int U> static constexpr PUnit pu() { return fixed_units(FIX).units[MEM][U]; }
    template <int U> static constexpr int items() { return pu<U>().a.items + pu<U>().b.items; }
    template <int U> __device__ __forceinline__ Unit unit() const {
        constexpr PUnit p = pu<U>();
        return Unit{bound(p.a, image), bound(p.b, image), p.epi, p.col0};
    }
    // weights of item `it` of unit U
    template <int U> __device__ __forceinline__ const float* weights(int it) const {
        constexpr PUnit p = pu<U>();
        if constexpr (p.b.items == 0) return lin_item_weights(bound(p.a, image), it);
        else if constexpr (p.a.items == 0) return lin_item_weights(bound(p.b, image), it);
        else return it >= p.a.items ? lin_item_weights(bound(p.b, image), it - p.a.items) : lin_item_weights(bound(p.a, image), it);
    }
    // the wave's first item in units U .. N - 1: its weights -> g; false: none
    template <int U> __device__ __forceinline__ bool first_from(int wave, const float*& g) const {
        if constexpr (U >= N) {
            return false;
        } else {
            if (wave < items<U>()) {
                g = weights<U>(wave);
                return true;
            }
            return first_from<U + 1>(wave, g);
        }
    }
    // the wave's item after item `it` of unit U
    template <int U> __device__ __forceinline__ bool next(int it, int wave, const float*& g) const {
        if constexpr (items<U>() > NWAVE) {
            if (it + NWAVE < items<U>()) {
                g = weights<U>(it + NWAVE);
                return true;
            }
        }
        return first_from<U + 1>(wave, g);
    }

    // kernel start: the wave's first item (none: the image's first chunks stand in for stream_load's unconditional loads)
    __device__ __forceinline__ void seek(Stream& st, int wave) const {
        st.iw.step = 0;
        st.g = image;
        st.live = first_from<0>(wave, st.g);
        st.g_next = st.g;
        st.has_next = false;
    }
    template <int U> __device__ __forceinline__ void begin_item(std::integral_constant<int, U>, Stream& st, int it, int wave) const {
        st.g_cur = weights<U>(it);
        st.g_next = st.g_cur;         // (no next item: RG > 1 re-reads this item's first chunks, as the run-time stream does)
        st.has_next = next<U>(it, wave, st.g_next);
    }
    // RG = 1.  Every item has 8 chunks; the last of them is issued while the multiply is in the same item, so g_next is its successor's
    __device__ __forceinline__ void issue(Stream& st, int) const {
        if (!st.live) return;
        issue_chunk(st.g + st.iw.step * CHUNK_FLOATS, st.ring_byte + (unsigned)st.islot * (CHUNK_FLOATS * 4), st.voff);
        ++st.issued;
        st.islot = st.islot == RING_SLOTS - 1 ? 0 : st.islot + 1;
        if (++st.iw.step == 8) {
            st.iw.step = 0;
            st.g = st.g_next;
            st.live = st.has_next;
        }
    }
    // RG > 1.  The round that multiplies chunks s0 .. s0 + 3 of the item refills the registers with the chunks RDEPTH further on: the
    // item's own, or -- in its last round -- the first RDEPTH of the next item
    __device__ __forceinline__ void begin_round(Stream& st, int chunks, int s0) const {
        st.g = s0 + RDEPTH < chunks ? st.g_cur + (s0 + RDEPTH) * CHUNK_FLOATS : st.g_next;
        st.iw.step = 0;
    }
    __device__ __forceinline__ void load(Stream& st, int, int lane, RChunk& c) const {
        const float* g = st.g + st.iw.step * CHUNK_FLOATS + lane * 4;
#pragma unroll
        for (int m = 0; m < 4; ++m) c.q[m] = *reinterpret_cast<const float4*>(g + 256 * m);
        ++st.iw.step;
    }
};

template <class F, int... I>
__device__ __forceinline__ void for_each_unit(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

// PRE: how the input rows are produced (compile-time: the three chains are three instantiations)
// FIX: -1 = the unit table is read from the kernel arguments (A = ChainArgs), else the fixed plan whose member MEM's table is compiled in
// (A = ChainArgsFx; `member` is then the constant MEM).  One body: the run-time and the fixed kernels differ in where a unit comes from.
template <int PRE, int RG, bool PAIR, int FIX, int MEM, class A>
__device__ __forceinline__ void chain_body(const A& a, const int pair, const int member) {
    using L = Lay<RG>;
    static_assert(!PAIR || (PRE == PRE_SLABS && RG > 1), "pair mode: the tail, wide row blocks");
    constexpr int R = L::R, RPW = L::RPW, OFF_X2 = L::OFF_X2, OFF_X3 = L::OFF_X3, OFF_H = L::OFF_H, OFF_C = L::OFF_C, OFF_R = L::OFF_R,
                  OFF_P = L::OFF_P, OFF_PARAM = L::OFF_PARAM;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // L::LDS_TOTAL_FLOATS (dynamic: > 64 KB)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const auto tab = [&] {
        if constexpr (FIX >= 0) return FxTab<FIX, MEM>{a.image};
        else return RtTab{a, (PAIR && member) ? a.units_b : a.units};
    }();
    constexpr int front_fx = fix_key(FIX < 0 ? 0 : FIX).with_front;
    unsigned* const pword = PAIR ? a.pair_sync + pair : nullptr;
    float* const px = PAIR ? a.pair_x + (long long)pair * (3 * R * DM) : nullptr;       // [3][R][256]
    const long long row0 = (long long)pair * R;
    float* P = smem + OFF_P;
    if constexpr (PRE == PRE_FRONT) {
        // prefix cache: the queries repeat bit for bit -> x and qkvt of the step that stored them stand; workgroup 0's first thread is the
        // single writer of the two counters
        if (a.skip_hdr) {
            const bool clean = sbev::prefix_clean(a.skip_hdr);
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                uint32_t* n = a.skip_hdr + (clean ? sbev::PFX_HITS : sbev::PFX_MISSES);
                *n = *n + 1u;
            }
            if (clean) return;
        }
    }
    if (PRE == PRE_ATT && a.zero_words && blockIdx.x == 0)
        for (int i = threadIdx.x; i < a.n_zero; i += 64 * NWAVE) a.zero_words[i] = 0u;

    // the weight stream starts before anything else: three chunks in flight
    SBEV_TRACE(0)
    warm_l2<RG>(a, wave, lane);
    Stream st;
    st.iw = Walk{0, wave, 0};
    st.issued = st.used = st.islot = st.uslot = 0;
    st.ring_byte = (unsigned)(L::OFF_RING + wave * (RING_SLOTS * CHUNK_FLOATS)) * 4u;
    st.voff = (unsigned)lane * 16u;
    st.g = a.warm;           // (valid for stream_load's unconditional loads even if this wave has no item)
    st.nchunk = 8;
    tab.seek(st, wave);
    RChunk rb[RDEPTH];
    if constexpr (L::WIDE) {
#pragma unroll
        for (int d = 0; d < RDEPTH; ++d) {
#pragma unroll
            for (int m = 0; m < 4; ++m) rb[d].q[m] = make_float4(0.f, 0.f, 0.f, 0.f);
            tab.load(st, wave, lane, rb[d]);
        }
    } else {
        tab.issue(st, wave);
        tab.issue(st, wave);
        tab.issue(st, wave);
    }

    // ---- prologue: every global load of it is issued before the first wait (one memory latency, not one per phase) -----
    const float* pv = smem + OFF_PARAM;
    constexpr int PASSES = (PV_FRONT_END / 4 + 64 * NWAVE - 1) / (64 * NWAVE);
    float4 pq[PASSES];                                   // the launch's small vectors, on their way to LDS
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
        const int i4 = (int)threadIdx.x + j * 64 * NWAVE;
        pq[j] = *reinterpret_cast<const float4*>(a.vec + 4 * min(i4, a.vec_n / 4 - 1));
    }
    // input rows: wave w owns rows w, w + 8 (RG = 4) of the workgroup
    float4 t[RPW], r4[RPW];
    float v0[RPW][4], v1[RPW][4];
    float bx[RPW], by[RPW], bz[RPW];
    bool plive[RPW];
#pragma unroll
    for (int pi = 0; pi < RPW; ++pi) {
        const int prow = wave + pi * NWAVE;
        const long long pg = row0 + prow;
        plive[pi] = prow < R && pg < a.M;
        t[pi] = make_float4(0.f, 0.f, 0.f, 0.f); r4[pi] = t[pi];
#pragma unroll
        for (int c = 0; c < 4; ++c) v0[pi][c] = v1[pi][c] = 0.f;
        bx[pi] = by[pi] = bz[pi] = 0.f;
        if (PRE == PRE_SLABS) {
            if (plive[pi]) r4[pi] = *reinterpret_cast<const float4*>(a.x1 + pg * DM + lane * 4);
        } else if (plive[pi]) {
            const float* src = PRE == PRE_FRONT ? a.feat : a.att;
#pragma unroll
            for (int c = 0; c < 4; ++c) v0[pi][c] = src[pg * DM + lane + 64 * c];
            if (PRE == PRE_FRONT) { bx[pi] = a.bbox[pg * 10]; by[pi] = a.bbox[pg * 10 + 1]; bz[pi] = a.bbox[pg * 10 + 2]; }
            if (PRE == PRE_ATT) {        // the residual of the out-projection: x rows, kept in LDS until the first epilogue
#pragma unroll
                for (int c = 0; c < 4; ++c) v1[pi][c] = a.x[pg * DM + lane + 64 * c];
            }
        }
    }
    if (PRE == PRE_SLABS) {
        // mixing.out_proj: sum of the split-K slabs -- up to 32 independent loads in flight per wave (all of its rows' together), added in
        // slab order; lane = 4 columns.  A dead row reads the last row's slabs (no branch: hipcc sinks loads into branches) x 0.
        constexpr int NB = 32 / RPW;             // (32 slabs = the fp16 out-projection's plan at 900 rows: one batch, one latency)
        for (int z0 = 0; z0 < a.splits; z0 += NB) {
            float4 q[RPW][NB];
#pragma unroll
            for (int pi = 0; pi < RPW; ++pi) {
                const long long pg = min(row0 + wave + pi * NWAVE, a.M - 1);
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    q[pi][j] = *reinterpret_cast<const float4*>(a.slabs + ((long long)min(z0 + j, a.splits - 1) * a.M + pg) * DM + lane * 4);
            }
#pragma unroll
            for (int pi = 0; pi < RPW; ++pi)
#pragma unroll
                for (int j = 0; j < NB; ++j) asm volatile("" ::"v"(q[pi][j].x), "v"(q[pi][j].y), "v"(q[pi][j].z), "v"(q[pi][j].w));   // all issued first
#pragma unroll
            for (int pi = 0; pi < RPW; ++pi)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const float m = (z0 + j < a.splits && plive[pi]) ? 1.f : 0.f;
                    t[pi].x += q[pi][j].x * m; t[pi].y += q[pi][j].y * m; t[pi].z += q[pi][j].z * m; t[pi].w += q[pi][j].w * m;
                }
        }
    }
#pragma unroll
    for (int j = 0; j < PASSES; ++j) asm volatile("" ::"v"(pq[j].x), "v"(pq[j].y), "v"(pq[j].z), "v"(pq[j].w));   // keeps the loads up there
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
        const int i4 = (int)threadIdx.x + j * 64 * NWAVE;
        if (i4 < a.vec_n / 4) *reinterpret_cast<float4*>(smem + OFF_PARAM + a.vec_off + 4 * i4) = pq[j];
    }
    __syncthreads();
#pragma unroll
    for (int pi = 0; pi < RPW; ++pi) {
        const int prow = wave + pi * NWAVE;
        if (prow >= R) continue;
        if (PRE == PRE_SLABS) {
            // + bias + residual x1 -> norm2 (sparsebev_transformer.py:171)
            float4 tt = t[pi];
            const float4 rr = r4[pi];
            const float4 b4 = *reinterpret_cast<const float4*>(pv + PV_OP_B + lane * 4);
            if (plive[pi]) { tt.x = (tt.x + b4.x) + rr.x; tt.y = (tt.y + b4.y) + rr.y; tt.z = (tt.z + b4.z) + rr.z; tt.w = (tt.w + b4.w) + rr.w; }
            const float mean = wsum((tt.x + tt.y) + (tt.z + tt.w)) * (1.f / DM);
            const float dx = tt.x - mean, dy = tt.y - mean, dz = tt.z - mean, dw = tt.w - mean;
            const float rstd = rsqrtf(wsum((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.f / DM) + a.eps);
            const float4 g4 = *reinterpret_cast<const float4*>(pv + PV_N2G + lane * 4);
            const float4 n4 = *reinterpret_cast<const float4*>(pv + PV_N2B + lane * 4);
            *reinterpret_cast<float4*>(smem + OFF_X2 + prow * LDX + lane * 4) =
                make_float4(dx * rstd * g4.x + n4.x, dy * rstd * g4.y + n4.y, dz * rstd * g4.z + n4.z, dw * rstd * g4.w + n4.w);
        } else {
            store_rows(smem, PRE == PRE_FRONT ? OFF_X3 : OFF_X2, LDX, prow, lane, v0[pi]);
            if (PRE == PRE_ATT) store_rows(smem, OFF_R, LDX, prow, lane, v1[pi]);
            if (PRE == PRE_FRONT) pe0_row<RG>(a, smem, prow, lane, bx[pi], by[pi], bz[pi]);
        }
    }
    __syncthreads();

    SBEV_TRACE(1)
    // one unit: its items, then its epilogue.  `only`: 1 / 2 = the unit is known at compile time to have items of Lin a / b alone
    // (every unit of today's fixed plans), 0 = choose per item
    const auto run_unit = [&](const Unit& un, const auto uc, const auto only) __attribute__((always_inline)) {
        constexpr int ONLY = decltype(only)::value;
        [[maybe_unused]] const int u = uc;      // (the trace stamps number by it)
        const int items = un.a.items + un.b.items;
#pragma nounroll
        for (int it = wave; it < items; it += NWAVE) {
            const bool second = ONLY == 0 ? it >= un.a.items : ONLY == 2;
            const Lin& l = ONLY == 1 ? un.a : ONLY == 2 ? un.b : second ? un.b : un.a;
            tab.begin_item(uc, st, it, wave);
            if constexpr (L::WIDE) mma_item_wide<RG>(tab, st, rb, l, it - (second ? un.a.items : 0), smem, it, lane, wave);
            else mma_item(tab, st, l, it - (second ? un.a.items : 0), smem, it, lane, wave);
        }
        SBEV_TRACE(2 + 4 * u)
        __syncthreads();
        SBEV_TRACE(3 + 4 * u)
        if constexpr (PAIR) {
            if (un.epi == EPI_FFN1) {
                // this member's partial sums of ffn.layers.1 (its k-half) -> exchange rows; lane = columns lane + 64 c, stored as one float4
                for (int row = wave; row < R; row += NWAVE) {
                    float v[4];
                    gather4_raw<R>(v, P, un.a.KH, row, lane);
                    pair_store4(px + (member * R + row) * DM + lane * 4, v);
                }
                pair_arrive(pword);
                pair_wait(pword, 2u);
            } else if (un.epi == EPI_PE3 && member == 0) {
                pair_wait(pword, 3u);      // member 1's x rows
            }
        }
        // ---- epilogue: task = (row, side); wave-local row ops ----------------------------------------------------------
        for (int task = wave; task < 2 * R; task += NWAVE) {
            const int row = task % R, side = task / R;
            const long long g = row0 + row;
            const bool live = g < a.M;
            float v[4];
            if (PAIR && side != member && (un.epi == EPI_FFN0 || un.epi == EPI_BR1 || un.epi == EPI_BR2 || un.epi == EPI_OUT)) continue;
            switch (un.epi) {
            case EPI_FFN0: {     // relu(x2 W0^T + b0): side = column half
                gather4<R>(v, P, 0, un.a.KH, PAIR ? 0 : side * 4, row, lane, pv + PV_FFN0_B, side * 256);
#pragma unroll
                for (int c = 0; c < 4; ++c) smem[OFF_H + row * LDH + side * 256 + lane + 64 * c] = fmaxf(v[c], 0.f);
            } break;
            case EPI_FFN1: {     // + x2 -> norm3 -> x3
                if (side) break;
                const LnW lw(pv + PV_N3G, pv + PV_N3B, lane);
                float res[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) res[c] = smem[OFF_X2 + row * LDX + lane + 64 * c];
                if constexpr (PAIR) {       // member 0's + member 1's partial sums, in that order in both members
                    float own[4], oth[4];
                    gather4_raw<R>(own, P, un.a.KH, row, lane);
                    pair_load4(px + ((1 - member) * R + row) * DM + lane * 4, oth);
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = ((member ? oth[c] : own[c]) + (member ? own[c] : oth[c])) + pv[PV_FFN1_B + lane + 64 * c];
                } else {
                    gather4<R>(v, P, 0, un.a.KH, 0, row, lane, pv + PV_FFN1_B, 0);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += res[c];
                ln4(v, lw, a.eps, false);
                store_rows(smem, OFF_X3, LDX, row, lane, v);
                if (live && member == 0) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.x3[g * DM + lane + 64 * c] = v[c];
                }
            } break;
            case EPI_BR1:        // cls_branch[0..2] | reg_branch[0..1]
            case EPI_BR2: {      // cls_branch[3..5] | reg_branch[2..3]
                const bool first = un.epi == EPI_BR1;
                if (side == 0) {
                    const LnW lw(pv + (first ? PV_CLS1G : PV_CLS4G), pv + (first ? PV_CLS1B : PV_CLS4B), lane);
                    gather4<R>(v, P, 0, un.a.KH, 0, row, lane, pv + (first ? PV_CLS0_B : PV_CLS3_B), 0);
                    ln4(v, lw, a.eps, true);
                    store_rows(smem, OFF_C, LDX, row, lane, v);
                } else {
                    gather4<R>(v, P, un.a.items, un.b.KH, 0, row, lane, pv + (first ? PV_REG0_B : PV_REG2_B), 0);
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], 0.f);
                    store_rows(smem, OFF_R, LDX, row, lane, v);
                }
            } break;
            case EPI_OUT: {      // cls_branch[6] -> scores | reg_branch[4] -> refine_bbox (:174-183) [-> next position encoder]
                if (side == 0) {
                    if (lane < a.num_classes) {
                        float s = 0.f;
                        for (int kh = 0; kh < un.a.KH; ++kh) s += P[kh * (R * 64) + row * 64 + lane];
                        if (live) a.cls_out[g * a.num_classes + lane] = s + pv[PV_CLS6_B + lane];
                    }
                } else {
                    float o = 0.f;
                    if (lane < 10) {
                        float s = 0.f;
                        for (int kh = 0; kh < un.b.KH; ++kh) s += P[(un.a.items + kh) * (R * 64) + row * 64 + lane];
                        const float r = s + pv[PV_REG4_B + lane];
                        const long long gi = live ? g : 0;
                        if (lane < 3) {
                            float p = a.bbox[gi * 10 + lane];
                            p = fminf(fmaxf(p, 0.f), 1.f);
                            const float logit = logf(fmaxf(p, 1e-5f) / fmaxf(1.f - p, 1e-5f));
                            o = 1.f / (1.f + expf(-(r + logit)));
                        } else {
                            o = r;
                            if (lane >= 8 && a.vel_div) o = r / a.vel_div[(unsigned)gi / (unsigned)a.Q];
                        }
                        if (live) a.box_out[g * 10 + lane] = o;
                    }
                    if (FIX >= 0 ? front_fx : a.front) {
                        const int ob = (int)__float_as_uint(o);
                        const float x0 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(ob, 0));
                        const float x1 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(ob, 1));
                        const float x2 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(ob, 2));
                        pe0_row<RG>(a, smem, row, lane, x0, x1, x2);
                    }
                }
            } break;
            case EPI_PE3: {      // position_encoder[3..5] + query_feat -> x (:166-167)
                if (side) break;
                if (PAIR && member == 0) {       // the x rows come from member 1
                    pair_load4(px + (2 * R + row) * DM + lane * 4, v);
                    store_rows(smem, OFF_X2, LDX, row, lane, v);
                    break;
                }
                const LnW lw(pv + PV_PE4G, pv + PV_PE4B, lane);
                float res[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) res[c] = smem[OFF_X3 + row * LDX + lane + 64 * c];
                gather4<R>(v, P, 0, un.a.KH, 0, row, lane, pv + PV_PE3_B, 0);
                ln4(v, lw, a.eps, true);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += res[c];
                store_rows(smem, OFF_X2, LDX, row, lane, v);
                if (PAIR) pair_store4(px + (2 * R + row) * DM + lane * 4, v);
                if (live) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.x[g * DM + lane + 64 * c] = v[c];
                }
            } break;
            case EPI_QKV: {      // attention in-projection + gen_tau rows -> qkvt
                const int ncg = un.a.items / un.a.KH;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int cg = side * 4 + c;
                    const int n = un.col0 + cg * 64 + lane;
                    if (cg < ncg && n < a.attn_in_rows) {
                        float s = 0.f;
                        for (int kh = 0; kh < un.a.KH; ++kh) s += P[(cg * un.a.KH + kh) * (R * 64) + row * 64 + lane];
                        if (live) a.qkvt[g * a.attn_in_rows + n] = s + pv[PV_QKV_B + n];
                    }
                }
            } break;
            case EPI_AOUT: {     // attention out-projection + x -> norm1 -> x1 (:169)
                if (side) break;
                const LnW lw(pv + PV_N1G, pv + PV_N1B, lane);
                float res[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) res[c] = smem[OFF_R + row * LDX + lane + 64 * c];     // x rows, staged by the prologue
                gather4<R>(v, P, 0, un.a.KH, 0, row, lane, pv + PV_AOUT_B, 0);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += res[c];
                ln4(v, lw, a.eps, false);
                store_rows(smem, OFF_X3, LDX, row, lane, v);
                if (live) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.x1_out[g * DM + lane + 64 * c] = v[c];
                }
                if (a.x1_frag && live) {
                    // the generator's operand, saving its pack launch (5 us per layer): lane = (image, 8-k piece) reads the piece's 8
                    // values of the row just written to LDS (same wave: the LDS pipe keeps its accesses in order) and stores 16 bytes
                    // at the piece's place in fragment (g / 32, k-step): row g % 32 is "lane" g % 32 + 32 (k-half) of that fragment
                    __builtin_amdgcn_wave_barrier();
                    const int k8 = lane & 31, im = lane >> 5;
                    const float up = a.x1_scale[0];
                    const float4 p0 = *reinterpret_cast<const float4*>(smem + OFF_X3 + row * LDX + 8 * k8);
                    const float4 p1 = *reinterpret_cast<const float4*>(smem + OFF_X3 + row * LDX + 8 * k8 + 4);
                    const float f[8] = {p0.x * up, p0.y * up, p0.z * up, p0.w * up, p1.x * up, p1.y * up, p1.z * up, p1.w * up};
                    unsigned w4[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const _Float16 h0 = (_Float16)f[2 * i], h1 = (_Float16)f[2 * i + 1];
                        const _Float16 l0 = (_Float16)(f[2 * i] - (float)h0), l1 = (_Float16)(f[2 * i + 1] - (float)h1);
                        const _Float16 e0 = im ? l0 : h0, e1 = im ? l1 : h1;
                        w4[i] = (unsigned)__builtin_bit_cast(unsigned short, e0) | ((unsigned)__builtin_bit_cast(unsigned short, e1) << 16);
                    }
                    const long long frag = ((g >> 5) * (DM / 16) + (k8 >> 1)) * 2 + im;            // [row block][k-step][image]
                    uint4* dst = reinterpret_cast<uint4*>(a.x1_frag + frag * 512 + (((int)(g & 31) + 32 * (k8 & 1)) * 8));
                    *dst = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                }
            } break;
            case EPI_SAMP: {     // sampling_offset | scale_weights Linear -> so (kept in LDS for the projection below)
                if (side) break;
                const int ncg = un.a.items / un.a.KH;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int n = c * 64 + lane;
                    if (c < ncg && n < a.soN) {
                        float s = 0.f;
                        for (int kh = 0; kh < un.a.KH; ++kh) s += P[(c * un.a.KH + kh) * (R * 64) + row * 64 + lane];
                        s += pv[PV_SAMP_B + n];
                        smem[OFF_H + row * 256 + n] = s;
                        if (live && a.so) a.so[g * a.soN + n] = s;
                    }
                }
            } break;
            }
        }
        SBEV_TRACE(4 + 4 * u)
        if (PAIR && un.epi == EPI_PE3 && member == 1) pair_arrive(pword);
        __syncthreads();
        SBEV_TRACE(5 + 4 * u)
    };
    if constexpr (FIX >= 0) {
        for_each_unit([&](const auto uc) __attribute__((always_inline)) {
            constexpr int UI = decltype(uc)::value;
            constexpr PUnit p = FxTab<FIX, MEM>::template pu<UI>();
            const Unit un = tab.template unit<UI>();
            run_unit(un, uc, std::integral_constant<int, p.b.items == 0 ? 1 : p.a.items == 0 ? 2 : 0>{});
        }, std::make_integer_sequence<int, FxTab<FIX, MEM>::N>{});
    } else {
        for (int u = 0; u < a.n_units; ++u) run_unit(tab.U[u], u, std::integral_constant<int, 0>{});
    }
    if (PRE == PRE_ATT && a.proj.loc_bp) {
        // adaptive spatio-temporal sampling, projection and camera selection of the rows' sample points (sample_point.hpp: the
        // same function as sample_project_kernel): thread = (frame t, group g, row, point p) -> 48-byte runs of loc_bp
        const int GP = a.proj.G * a.proj.P;
        for (int i = threadIdx.x; i < R * a.proj.T * GP; i += 64 * NWAVE) {
            const int p = i % a.proj.P;
            const int row = (i / a.proj.P) % R;
            const int tg = i / (a.proj.P * R);
            const int gq = tg % a.proj.G, t = tg / a.proj.G;
            const long long g = row0 + row;
            if (g >= a.M) continue;
            const int b = (int)((unsigned)g / (unsigned)a.Q), q = (int)((unsigned)g - (unsigned)b * (unsigned)a.Q);
            const int gp = gq * a.proj.P + p;
            const float* so = smem + OFF_H + row * 256;
            sbev_ops::sample_point(a.proj, b, t, q, gp, a.proj.bbox + g * 10, so + gp * 3, so + GP * 3 + gp * a.proj.L);
        }
    }
}

// pair mode: block b -> XCD b % 8 under round-robin dispatch, so the members of pair p are blocks b and b + 8.  False: this
// workgroup has no pair (or is the member the test hook drops)
template <bool PAIR>
__device__ __forceinline__ bool pair_of_block(const ChainCommon& a, int& pair, int& member) {
    pair = (int)blockIdx.x;
    member = 0;
    if constexpr (PAIR) {
        const int li = (int)blockIdx.x >> 3;
        pair = (li >> 1) * 8 + ((int)blockIdx.x & 7);
        member = li & 1;
        if (pair >= a.n_pairs) return false;
        if (a.debug_drop && pair == 0 && member == 1) return false;
    }
    return true;
}

template <int PRE, int RG, bool PAIR = false>
__global__ __launch_bounds__(64 * NWAVE) void row_chain_kernel(const ChainArgs a) {
    int pair, member;
    if (!pair_of_block<PAIR>(a, pair, member)) return;
    chain_body<PRE, RG, PAIR, -1, -1>(a, pair, member);
}

// the same chain with fixed plan FIX compiled in; a pair's two members run two instantiations of the body, one per table
template <int PRE, int RG, bool PAIR, int FIX>
__global__ __launch_bounds__(64 * NWAVE) void row_chain_fixed_kernel(const ChainArgsFx a) {
    int pair, member;
    if (!pair_of_block<PAIR>(a, pair, member)) return;
    if constexpr (PAIR) {
        if (member == 0) chain_body<PRE, RG, PAIR, FIX, 0>(a, pair, 0);
        else chain_body<PRE, RG, PAIR, FIX, 1>(a, pair, 1);
    } else {
        chain_body<PRE, RG, PAIR, FIX, 0>(a, pair, 0);
    }
}

// weights [N, K] row-major (ld) -> the order the lanes consume them: [ceil(N/64)][K/16][4][64 lanes][4 floats],
// lane = column within the group, (step, m, e) -> k = 16 step + 4 m + e; rows past N are zero
__global__ void pack_kernel(const float* W, long long ld, int N, int K, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // one float4 each
    const long long total = (long long)((N + 63) / 64) * K * 16;
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const long long t = i >> 6;
    const int m = (int)(t & 3);
    const long long t2 = t >> 2;
    const int steps = K / 16;
    const int s = (int)(t2 % steps);
    const int cg = (int)(t2 / steps);
    const int n = cg * 64 + lane;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N) v = *reinterpret_cast<const float4*>(W + (long long)n * ld + 16 * s + 4 * m);
    reinterpret_cast<float4*>(out)[i] = v;
}

__global__ void copy_pad_kernel(const float* src, int n, float* dst, int slot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < slot) dst[i] = i < n ? src[i] : 0.f;
}

// ======================================================= host side =======================================================================
// ---- the instantiations, listed once ------------------------------------------------------------------------------------------------------
// launch, the LDS-attribute raise and chain_lds_ready walk this table.  The kernels use 159 KB of dynamic LDS: the attribute is raised once
// per device and instantiation (also from sbev_decoder_chain_pack, so that the first launch may already be inside a stream capture).
struct Inst {
    int pre, rg;
    bool pair;
    int fix;                                         // -1: the run-time-table kernel (kern); else the fixed plan compiled into kern_fx
    void (*kern)(ChainArgs);
    void (*kern_fx)(ChainArgsFx);
    int rows, lds;                                   // rows per row block (one workgroup, or one pair of them); dynamic LDS bytes
    std::atomic<unsigned long long> raised;          // bit d: the attribute is raised on device d (a process may drive several devices)
};
template <int PRE, int RG, bool PAIR = false>
Inst inst() { return Inst{PRE, RG, PAIR, -1, row_chain_kernel<PRE, RG, PAIR>, nullptr, Lay<RG>::R, Lay<RG>::LDS_TOTAL_FLOATS * 4, {0}}; }
template <int FIX>
Inst inst_fixed() {
    constexpr FixKey k = fix_key(FIX);
    return Inst{k.pre, k.rg, k.pair != 0, FIX, nullptr, row_chain_fixed_kernel<k.pre, k.rg, k.pair != 0, FIX>, Lay<k.rg>::R,
                Lay<k.rg>::LDS_TOTAL_FLOATS * 4, {0}};
}
Inst kInst[] = {inst<PRE_SLABS, 1>(), inst<PRE_FRONT, 1>(), inst<PRE_ATT, 1>(), inst<PRE_SLABS, 2>(), inst<PRE_FRONT, 2>(), inst<PRE_ATT, 2>(),
                inst<PRE_SLABS, 4>(), inst<PRE_FRONT, 4>(), inst<PRE_ATT, 4>(), inst<PRE_SLABS, 2, true>(), inst<PRE_SLABS, 4, true>(),
                inst_fixed<0>(), inst_fixed<1>(), inst_fixed<2>(), inst_fixed<3>()};
static_assert(N_FIX == 4, "one inst_fixed row per fixed plan");
Inst* find_inst(int pre, int rg, bool pair, int fix = -1) {
    for (Inst& i : kInst)
        if (i.pre == pre && i.rg == rg && i.pair == pair && i.fix == fix) return &i;
    return nullptr;
}
hipError_t raise_lds(Inst& i) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    const unsigned long long bit = 1ull << (dev & 63);
    if (i.raised.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(i.fix < 0 ? reinterpret_cast<const void*>(i.kern) : reinterpret_cast<const void*>(i.kern_fx), hipFuncAttributeMaxDynamicSharedMemorySize, i.lds);
    if (e == hipSuccess) i.raised.fetch_or(bit, std::memory_order_release);
    return e;
}

// ---- a launch, planned once (pure host: no HIP call below this line until "binding and launching") ----------------------------------
struct ChainPlan : PlanUnits {   // (the unit tables: n_units, units[member][u])
    int pre, rg, pair;           // the instantiation: the chain (Pre), row groups per row block, pair mode
    unsigned grid;
    int lds;                     // dynamic LDS bytes
    int n_pairs;
    long long warm;              // the launch's packed weights: float offset of the span, ...
    int warm_lines;              // ... its 128-byte lines
    long long vec;               // the launch's small vectors: float offset in the image -> LDS parameter block [vec_off, vec_off + vec_n)
    int vec_off, vec_n;
};

// rows per workgroup = 4 rg: the smallest of 4, 8, 16 that covers the rows with one round of workgroups (256 CUs)
int row_groups(long long rows) {
    static const int forced = getenv("SBEV_CHAIN_RG") ? atoi(getenv("SBEV_CHAIN_RG")) : 0;      // A/B: 1, 2 or 4 row groups whatever the row count
    if ((forced == 1 && rows <= 256 * 4) || (forced == 2 && rows <= 256 * 8) || forced == 4) return forced;
    return rows <= 256 * 4 ? 1 : rows <= 256 * 8 ? 2 : 4;
}
// Pair mode of the tail (see "pair mode" above): row groups per PAIR of workgroups, 0 = not applicable.  Both members of every
// pair must be resident at once -- one workgroup per CU (88 KB of LDS and more) -- so the launch, 16 blocks per 8 pairs, has to
// fit the device's CUs in one round: 8 rows per pair, <= 1024 rows on 256 CUs.  (16 rows per pair would reach 2048 rows, but
// four row groups per weight chunk are MFMA-bound, not stream-bound: 88 vs 66 us for the single-workgroup tail at 1600 rows;
// SBEV_CHAIN_PAIR16=1 enables it for A/B runs.)  pair_ok: the switch is on, the fault word is installed (no other way to report a
// lost partner) and the caller gave the exchange workspace.
int pair_blocks(long long rows, int rg) {
    const long long pairs = (rows + 4 * rg - 1) / (4 * rg);
    return (int)(16 * ((pairs + 7) / 8));
}
int pair_row_groups(long long rows, bool pair_ok, int cus) {
    if (!pair_ok || rows > 256 * 16) return 0;
    static const int max_rg = getenv("SBEV_CHAIN_PAIR16") ? 4 : 2;
    for (int rg = 2; rg <= max_rg; rg *= 2)
        if (pair_blocks(rows, rg) <= cus) return rg;
    return 0;
}

// Everything a row-chain launch needs but its pointers, from plain values (sbev_decoder_chain_plan reports it; tests/test_chain_plan_host.py).
// pre: the chain; with_front: the tail goes on with the next layer's front; pair_ok: see pair_row_groups; cus: the device's CU count
ChainPlan chain_plan(const Cfg& c, int pre, bool with_front, bool pair_ok, int cus) {
    const long long rows = (long long)c.B * c.Q;
    const PackMap m = pack_map(c);
    ChainPlan p{};
    p.pre = pre;
    const int prg = pre == PRE_SLABS ? pair_row_groups(rows, pair_ok, cus) : 0;
    p.pair = prg != 0;
    p.rg = p.pair ? prg : row_groups(rows);
    const Inst& in = *find_inst(p.pre, p.rg, p.pair);
    const long long blocks = (rows + in.rows - 1) / in.rows;
    p.grid = p.pair ? (unsigned)pair_blocks(rows, p.rg) : (unsigned)blocks;
    p.lds = in.lds;
    p.n_pairs = p.pair ? (int)blocks : 0;
    static const Tweaks tw{getenv("SBEV_CHAIN_TIE_SMALL") == nullptr, getenv("SBEV_CHAIN_PAIR_Q0") ? atoi(getenv("SBEV_CHAIN_PAIR_Q0")) : -1};      // A/B
    static_cast<PlanUnits&>(p) = plan_units(c, pre, p.rg, p.pair != 0, with_front, tw);
    int first = 0, last = 0;         // the launch streams matrices first .. last: one contiguous span of the image
    if (pre == PRE_FRONT) {
        first = M_PE3; last = M_ATTN_IN;
        p.vec = m.vec() + PV_TAIL_END; p.vec_off = PV_TAIL_END; p.vec_n = PV_FRONT_END - PV_TAIL_END;
    } else if (pre == PRE_ATT) {
        first = M_ATTN_OUT; last = M_SAMP;
        p.vec = m.vec() + PV_FRONT_END; p.vec_off = 0; p.vec_n = PV_ATTN_END;
    } else {
        first = M_FFN0; last = with_front ? M_ATTN_IN : M_REG4;
        p.vec = m.vec(); p.vec_off = 0; p.vec_n = with_front ? PV_FRONT_END : PV_TAIL_END;
    }
    p.warm = m.at[first];
    p.warm_lines = m.lines(first, last);
    return p;
}

std::atomic<int> g_chain_pair{getenv("SBEV_NO_CHAIN_PAIR") ? 0 : 1};
std::atomic<int> g_chain_pair_drop{0};

// ---- choosing a fixed plan ---------------------------------------------------------------------------------------------------------------------
constexpr PlanUnits kFixedUnits[N_FIX] = {fixed_units(0), fixed_units(1), fixed_units(2), fixed_units(3)};
// the fixed kernels are taken (default) / only the run-time-table kernels are (sbev_decoder_chain_fixed, SBEV_CHAIN_FIXED=0)
std::atomic<int> g_chain_fixed{getenv("SBEV_CHAIN_FIXED") ? (atoi(getenv("SBEV_CHAIN_FIXED")) != 0 ? 1 : 0) : 1};
std::atomic<long long> g_chain_fixed_launches{0};      // launches (enqueued or captured) that took a fixed kernel, for tests

// a unit as the 18 int32 words sbev_decoder_chain_plan reports (and fixed_match compares)
void unit_words(const PUnit& pu, int32_t* out) {
    *out++ = pu.epi;
    *out++ = pu.col0;
    for (const PLin* l : {&pu.a, &pu.b})
        for (int v : {(int)l->w, l->in_off, l->ld, l->KH, l->items, l->chunks, l->kh0, l->KHT}) *out++ = v;
}
// the key of a planned launch
FixKey key_of(const Cfg& c, const ChainPlan& p, bool with_front) {
    return FixKey{p.pre, p.rg, p.pair, p.pre == PRE_SLABS && with_front ? 1 : 0, (c.attn_in_rows + 63) / 64, (so_cols(c) + 63) / 64};
}
// the fixed plan with this key, -1: none is compiled in
int find_fixed(const FixKey& k) {
    for (int i = 0; i < N_FIX; ++i)
        if (same_key(fix_key(i), k)) return i;
    return -1;
}
// ... and whose constant table equals the plan's run-time table word for word (it does, unless an A/B switch of the environment changed
// the plan: the key does not know those), -1: the launch takes the run-time-table kernel
int fixed_match(const ChainPlan& p, const FixKey& k) {
    static const bool ab_env = getenv("SBEV_CHAIN_TIE_SMALL") || getenv("SBEV_CHAIN_PAIR_Q0") || getenv("SBEV_CHAIN_RG") || getenv("SBEV_CHAIN_PAIR16");
    const int fix = ab_env ? -1 : find_fixed(k);
    if (fix < 0 || kFixedUnits[fix].n_units != p.n_units) return -1;
    for (int mem = 0; mem <= p.pair; ++mem)
        for (int u = 0; u < p.n_units; ++u) {
            int32_t a[18], b[18];
            unit_words(p.units[mem][u], a);
            unit_words(kFixedUnits[fix].units[mem][u], b);
            if (memcmp(a, b, sizeof(a)) != 0) return -1;
        }
    return fix;
}

int device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    int v = cus[dev & 63].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cus[dev & 63].store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace

namespace sbev {

// pair mode workspace: exchange rows (floats) and arrival counters (words) for `rows` rows, whatever the row block it picks
long long chain_pair_floats(long long rows) { return 3 * (rows + 15) * DM; }
// (+ 64 words behind the pair counters: the out-projection's fold counters, one per row tile -- zeroed by the same attention-chain loop)
long long chain_pair_sync_words(long long rows) { return (rows + 7) / 8 + 64; }
long long chain_fold_sync_offset(long long rows) { return (rows + 7) / 8; }
bool chain_pair_enabled() { return g_chain_pair.load(std::memory_order_relaxed) != 0; }

// this file's end of the decoder's sticky fault word (fault_word.hip): the device address of the host-mapped word for the pair hand-off's
// timeout path, and the device-side count of those timeouts (-1: HIP error; synchronises the device)
bool chain_pair_install(void* host_word_dev) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_chain_pair_fault_host), &host_word_dev, sizeof(host_word_dev)) == hipSuccess;
}
long long chain_pair_timeouts() {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_chain_pair_timeouts), sizeof(v)) != hipSuccess) return -1;
    return (long long)v;
}

bool row_chain_supported(const sbev_decoder_config& c) {
    return c.D == DM && c.ffn == FF && c.code_size == 10 && c.num_classes >= 1 && c.num_classes <= 64 &&
           c.attn_in_rows <= PV_QKV_PAD && so_cols(c) <= 256 && (long long)c.B * c.Q < 0x7fffffffLL;
}

// Every workgroup streams every weight: that pays while the launch is a single round of workgroups (<= 256 CUs).
// Measured (samples/s with / without the chains), 4 rows per workgroup: config 2 (900 rows) 350 / 328, config 5 387 / 358; config 3
// (3200 rows) 747 / 755, config 4 (3600 rows) 271 / 272 -- so larger batches take 8 or 16 rows per workgroup (round 3), and beyond
// 4096 rows the op-by-op launches, whose tiles amortise the weights, stay.  SBEV_CHAIN_MAX_ROWS overrides the limit (A/B).
bool row_chain_pays(long long rows) {
    static const long long limit = getenv("SBEV_CHAIN_MAX_ROWS") ? atoll(getenv("SBEV_CHAIN_MAX_ROWS")) : 256 * 16;
    return rows <= limit && rows <= 256 * 16;
}

bool chain_lds_ready() {
    for (Inst& i : kInst)
        if (raise_lds(i) != hipSuccess) return false;
    return true;
}

// ---- binding and launching: the plan's offsets onto the image, the activations, the kernel ----------------------------------------
static ChainArgs chain_args(const Cfg& c, float eps) {
    ChainArgs a{};
    a.M = (long long)c.B * c.Q;
    a.Q = c.Q;
    a.eps = eps;
    a.num_classes = c.num_classes;
    a.attn_in_rows = c.attn_in_rows;
    a.soN = so_cols(c);
    return a;
}

static int launch(const Cfg& c, const ChainPlan& p, ChainArgs& a, const float* pk, hipStream_t s, const char* what) {
    const int fix = g_chain_fixed.load(std::memory_order_relaxed) ? fixed_match(p, key_of(c, p, a.front != 0)) : -1;
    Inst& in = *find_inst(p.pre, p.rg, p.pair, fix);
    const hipError_t attr = raise_lds(in);
    if (attr != hipSuccess) {
        set_error("%s: hipFuncSetAttribute(%d bytes of LDS): %s", what, in.lds, hipGetErrorString(attr));
        return SBEV_ELAUNCH;
    }
    for (int mem = 0; mem <= p.pair; ++mem)
        for (int u = 0; u < p.n_units; ++u) {
            const PUnit& pu = p.units[mem][u];
            (mem ? a.units_b : a.units)[u] = Unit{bound(pu.a, pk), bound(pu.b, pk), pu.epi, pu.col0};
        }
    a.n_units = p.n_units;
    a.pre = p.pre;
    a.n_pairs = p.n_pairs;
    static const bool no_warm = getenv("SBEV_CHAIN_NO_WARM") != nullptr;       // A/B switch
    a.warm = pk + p.warm;
    a.warm_lines = no_warm ? 0 : p.warm_lines;
    a.vec = pk + p.vec; a.vec_off = p.vec_off; a.vec_n = p.vec_n;
#ifdef SBEV_CHAIN_TRACE
    static long long* tr = nullptr;
    static int calls = 0;
    static const Inst* who[13];
    if (!tr) { (void)hipMalloc(&tr, 2 * 64 * 8 * 8 * 64); (void)hipMemset(tr, 0, 2 * 64 * 8 * 8 * 64); }
    a.trace = tr + (calls % 64) * 512;
    if (calls < 13) who[calls] = &in;
#endif
    if (fix >= 0) {
        ChainArgsFx f{};
        static_cast<ChainCommon&>(f) = a;
        f.image = pk;
        g_chain_fixed_launches.fetch_add(1, std::memory_order_relaxed);
        hipLaunchKernelGGL(in.kern_fx, dim3(p.grid), dim3(64 * NWAVE), in.lds, s, f);
    } else {
        hipLaunchKernelGGL(in.kern, dim3(p.grid), dim3(64 * NWAVE), in.lds, s, a);
    }
#ifdef SBEV_CHAIN_TRACE
    if (++calls == 13) {        // the first step's 13 launches
        (void)hipDeviceSynchronize();
        static long long h[2 * 64 * 512];
        (void)hipMemcpy(h, tr, sizeof(h), hipMemcpyDeviceToHost);
        for (int c = 0; c < 13; ++c) {
            const long long* t = h + c * 512;
            printf("launch %d (PRE %d RG %d PAIR %d; 10 ns ticks):", c, who[c]->pre, who[c]->rg, (int)who[c]->pair);
            for (int blk = 0; blk < 2; ++blk)
                for (int w = 0; w < 8; w += 7) {
                    const long long* tb = t + blk * 64 * 512;
                    printf(" [b%d w%d]", blk ? 15 : 7, w);
                    for (int i = 0; i < 2 + 4 * 8 && tb[w * 64 + i]; ++i) printf(" %lld", tb[w * 64 + i] - t[0]);
                }
            printf("\n");
        }
    }
#endif
    return check_launch(what);
}

// position encoder + attention in-projection of the FIRST layer (the later layers' run at the end of the previous tail)
int launch_chain_front(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* bbox, const float* feat, float* x,
                       float* qkvt, float eps, hipStream_t s, uint32_t* skip_hdr) {
    ChainArgs a = chain_args(c, eps);
    a.bbox = bbox; a.feat = feat; a.x = x; a.qkvt = qkvt; a.skip_hdr = skip_hdr;
    return launch(c, chain_plan(c, PRE_FRONT, false, false, 0), a, w.chain_pack, s, "row chain (front)");
}

// attention out-projection + residual + norm1 -> x1, sampling Linear -> sample points -> projection (loc, level weights)
int launch_chain_attn(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* att, const float* x, float* x1,
                      const float* bbox, const float* time_diff, const float* lidar2img, float* loc_bp, float* w_bp, float eps,
                      hipStream_t s, uint16_t* x1_frag, const float* x1_scale, uint32_t* pair_sync, const LazyPlan* touch, uint32_t* touch_need) {
    ChainArgs a = chain_args(c, eps);
    a.zero_words = pair_sync;            // the arrival counters of this layer's tail (pair mode), zeroed here: chain_pair_sync_words()
    a.n_zero = pair_sync ? (int)chain_pair_sync_words(a.M) : 0;
    a.att = att; a.x = const_cast<float*>(x); a.x1_out = x1; a.so = nullptr;
    a.x1_frag = x1_frag; a.x1_scale = x1_scale;
    a.proj = sbev_ops::sample_point_args(bbox, time_diff, lidar2img, c.pc_range, c.B, c.Q, c.T, c.N, c.G, c.P, c.L, c.image_h, c.image_w,
                                         c.eps_homo, loc_bp, w_bp);
    if (touch && touch_need) sbev_ops::sample_point_touch(a.proj, *touch, c.hw, touch_need);      // on-demand relayout: mark what the points read
    return launch(c, chain_plan(c, PRE_ATT, false, false, 0), a, w.chain_pack, s, "row chain (attention)");
}

// out_proj slabs -> norm2 -> ffn -> norm3 -> branches -> refine_bbox [-> the next layer's position encoder + in-projection]
int launch_chain_tail(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* slabs, int splits, const float* x1,
                      const float* bbox, const float* vel_div, float* x3, float* cls_out, float* box_out, int with_front, float* x,
                      float* qkvt, float eps, hipStream_t s, float* pair_x, uint32_t* pair_sync) {
    ChainArgs a = chain_args(c, eps);
    a.slabs = slabs; a.splits = splits; a.x1 = x1; a.bbox = bbox; a.vel_div = vel_div;
    a.x3 = x3; a.cls_out = cls_out; a.box_out = box_out; a.front = with_front; a.x = x; a.qkvt = qkvt;
    // pair mode: allowed while the switch is on, the workspace was given and a lost partner can be reported (the fault word is installed)
    const bool pair_ok = pair_x && pair_sync && chain_pair_enabled() && a.M <= 256 * 16 && chain_fault_word_ready();
    const ChainPlan p = chain_plan(c, PRE_SLABS, with_front != 0, pair_ok, pair_ok ? device_cus() : 0);
    if (p.pair) {
        a.pair_x = pair_x;
        a.pair_sync = pair_sync;
        a.debug_drop = g_chain_pair_drop.load(std::memory_order_relaxed);
    }
    return launch(c, p, a, w.chain_pack, s, p.pair ? "row chain (tail, pairs)" : "row chain (tail)");
}

}  // namespace sbev

// pair mode of the tail: on (default) / off; returns the previous setting (A/B measurements, tests)
extern "C" int sbev_decoder_chain_pair(int enable) { return g_chain_pair.exchange(enable != 0 ? 1 : 0); }

// TEST HOOK: with 1, member 1 of pair 0 of every pair-mode tail exits at once, so that its partner runs into the poll bound (the rows
// of that pair are garbage, every other row is unaffected, the launch ends); returns the previous setting
extern "C" int sbev_debug_chain_pair_drop(int enable) { return g_chain_pair_drop.exchange(enable != 0 ? 1 : 0); }

extern "C" int64_t sbev_decoder_chain_pack_floats(const sbev_decoder_config* cfg) {
    if (!cfg || !sbev::row_chain_supported(*cfg)) return 0;
    return pack_map(*cfg).total();
}

// the fixed-plan kernels: on / off; returns the previous setting (A/B measurements, tests).  Results are bit-identical either way
extern "C" int sbev_decoder_chain_fixed(int enable) { return g_chain_fixed.exchange(enable != 0 ? 1 : 0); }
extern "C" int64_t sbev_decoder_chain_fixed_launches(void) { return g_chain_fixed_launches.load(std::memory_order_relaxed); }

// a plan's int32 words (layout: include/sbev_hip.h): its header, then `t`'s unit tables
static int plan_words(const ChainPlan& p, const PlanUnits& t, int32_t* out, int capacity, const char* who) {
    const int members = p.pair ? 2 : 1;
    const long long words = 12 + 18LL * members * t.n_units;
    SBEV_REQUIRE(out && capacity >= words, "%s: %lld words needed", who, words);
    for (int v : {p.pre, p.rg, p.pair, (int)p.grid, p.lds, t.n_units, p.n_pairs, (int)p.warm, p.warm_lines, (int)p.vec, p.vec_off, p.vec_n}) *out++ = v;
    for (int mem = 0; mem < members; ++mem)
        for (int u = 0; u < t.n_units; ++u, out += 18) unit_words(t.units[mem][u], out);
    return (int)words;
}

static bool plan_args_ok(const sbev_decoder_config* cfg, int kind, int cus) {
    return cfg && sbev::row_chain_supported(*cfg) && cfg->B >= 1 && cfg->Q >= 1 && (long long)cfg->B * cfg->Q <= 256 * 16 && kind >= PRE_SLABS &&
           kind <= PRE_ATT && cus >= 0;
}

// The same launch as a fixed plan would run it: the header of chain_plan, the unit tables from the constant table of the fixed kernel
// with the launch's key.  0 = none: no fixed kernel has that key (or the config is not covered by the row chains at all).  Touches no device
extern "C" int sbev_decoder_chain_fixed_plan(const sbev_decoder_config* cfg, int kind, int with_front, int pair_ok, int cus, int32_t* out, int capacity) {
    if (!plan_args_ok(cfg, kind, cus)) return 0;
    const ChainPlan p = chain_plan(*cfg, kind, with_front != 0, pair_ok != 0, cus);
    const int fix = find_fixed(key_of(*cfg, p, with_front != 0));
    if (fix < 0) return 0;
    return plan_words(p, kFixedUnits[fix], out, capacity, "sbev_decoder_chain_fixed_plan");
}

// chain_plan's answer as int32 words (layout: include/sbev_hip.h).  Touches no device
extern "C" int sbev_decoder_chain_plan(const sbev_decoder_config* cfg, int kind, int with_front, int pair_ok, int cus, int32_t* out, int capacity) {
    SBEV_REQUIRE(plan_args_ok(cfg, kind, cus),
                 "sbev_decoder_chain_plan: config not covered by the row chains (1 .. 4096 rows), or kind / cus out of range");
    const ChainPlan p = chain_plan(*cfg, kind, with_front != 0, pair_ok != 0, cus);
    return plan_words(p, p, out, capacity, "sbev_decoder_chain_plan");
}

extern "C" int sbev_decoder_chain_pack(const sbev_decoder_config* cfg, const sbev_decoder_weights* w, float* out, sbev_stream_t stream) {
    SBEV_REQUIRE(cfg && w && out, "sbev_decoder_chain_pack: null pointer");
    SBEV_REQUIRE(sbev::row_chain_supported(*cfg), "sbev_decoder_chain_pack: config not covered by the row-chain kernels (embed_dims 256, ffn 512, code_size 10)");
    SBEV_REQUIRE((((uintptr_t)out) & 15) == 0, "sbev_decoder_chain_pack: output must be 16-byte aligned");
    const sbev_decoder_config& c = *cfg;
    const PackMap m = pack_map(c);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SBEV_REQUIRE(sbev::chain_lds_ready(), "sbev_decoder_chain_pack: the device refuses %d bytes of LDS per workgroup", Lay<1>::LDS_TOTAL_FLOATS * 4);
    for (int i = 0; i < N_MAT; ++i) {
        const float* W = w->*kMats[i].w;
        const int N = kMats[i].N(c), K = kMats[i].K(c);
        SBEV_REQUIRE(W && (((uintptr_t)W) & 15) == 0, "sbev_decoder_chain_pack: null / unaligned weight");
        const long long n4 = (long long)((N + 63) / 64) * K * 16;
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, W, (long long)K, N, K, out + m.at[i]);
    }
    // the small vectors, zero-padded to their slots
    float* pv = out + m.vec();
    struct Vec { const float* p; int off, n, slot; };
    const int soN = so_cols(c);
    const Vec vecs[] = {
        {w->op_b, PV_OP_B, c.D, 256}, {w->norm2_g, PV_N2G, c.D, 256}, {w->norm2_b, PV_N2B, c.D, 256}, {w->ffn0_b, PV_FFN0_B, c.ffn, 512},
        {w->ffn1_b, PV_FFN1_B, c.D, 256}, {w->norm3_g, PV_N3G, c.D, 256}, {w->norm3_b, PV_N3B, c.D, 256},
        {w->cls0_b, PV_CLS0_B, c.D, 256}, {w->cls1_g, PV_CLS1G, c.D, 256}, {w->cls1_b, PV_CLS1B, c.D, 256},
        {w->cls3_b, PV_CLS3_B, c.D, 256}, {w->cls4_g, PV_CLS4G, c.D, 256}, {w->cls4_b, PV_CLS4B, c.D, 256},
        {w->cls6_b, PV_CLS6_B, c.num_classes, 64}, {w->reg0_b, PV_REG0_B, c.D, 256}, {w->reg2_b, PV_REG2_B, c.D, 256},
        {w->reg4_b, PV_REG4_B, c.code_size, 64},
        {w->pe0_w, PV_PE0_W, 3 * c.D, 768}, {w->pe0_b, PV_PE0_B, c.D, 256}, {w->pe1_g, PV_PE1G, c.D, 256}, {w->pe1_b, PV_PE1B, c.D, 256},
        {w->pe3_b, PV_PE3_B, c.D, 256}, {w->pe4_g, PV_PE4G, c.D, 256}, {w->pe4_b, PV_PE4B, c.D, 256},
        {w->attn_in_b, PV_QKV_B, c.attn_in_rows, PV_QKV_PAD},
        {w->attn_out_b, PV_FRONT_END + PV_AOUT_B, c.D, 256}, {w->norm1_g, PV_FRONT_END + PV_N1G, c.D, 256},
        {w->norm1_b, PV_FRONT_END + PV_N1B, c.D, 256}, {w->samp_b, PV_FRONT_END + PV_SAMP_B, soN, 256}};
    for (const Vec& v : vecs) {
        SBEV_REQUIRE(v.p, "sbev_decoder_chain_pack: null bias / LayerNorm pointer");
        hipLaunchKernelGGL(copy_pad_kernel, dim3((unsigned)((v.slot + 255) / 256)), dim3(256), 0, s, v.p, v.n, pv + v.off, v.slot);
    }
    return sbev::check_launch("sbev_decoder_chain_pack");
}
