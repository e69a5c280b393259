// phx_reduce.h — the PH reductions' device code: Compute_Xbar, Update_W and
// convergence_diff, the expectations, the adaptive-rho and cost-proportional-rho
// statistics.  Included once by phx_kernels.hip
// (after phx_core.h, phx_lane.h and `using namespace phx`), which keeps the
// context, the entry points and every launch.
//
// Two skeletons are written once here, and a new reduction adds an operation
// type to one of them, not a kernel body:
//   * per-node tile reduction (tile_pass, fold_all): k_xbar, k_absdev,
//     k_cost_rho_stats -- operations XbarOp, AbsdevOp, CostRhoOp;
//   * per-scenario scalar sums (sums_one_block, sums_part, k_expect_fold /
//     k_sums_fold): phx_expect, phx_rho_sums, phx_w_absdiff, Iter0's keep
//     kernels -- terms ExpectTerm, RhoTerm, WAbsdiffTerm.
// All reductions are fixed-order trees (no float atomics).
// The norm-rho update inside the device loop (phx_iterk_norm_rho) adds no
// reduction: its kernels are the absdev passes, the rule and the scale under a
// gate of their own (rho_gated), the rule evaluated by the block that holds
// every entry when the residuals need no all-reduce.
#pragma once

// ---- block reduction helpers (wave shuffles + LDS, fixed order) ----
template <int NT>
__device__ double block_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        for (int w = 0; w < NT / 64; ++w) r += sh[w];
    }
    __syncthreads();
    return r;   // valid in thread 0
}

#define RED_NT 256
// store_wt / load_wt / arrive_last (fence-free inter-workgroup hand-off) and
// the TICKET_* layout live in phx_lane.h (the fused lane kernels use them too)
using phx_lane::store_wt;
using phx_lane::load_wt;
using phx_lane::arrive_last;

// K sums over the block at once (wave shuffles, then the waves in order):
// one barrier pair for K values.  Results valid in thread 0.
template <int NT, int K>
__device__ void block_sum_multi(double (&v)[K], double* sh) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wid * K + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double r = 0.0;
            for (int w = 0; w < NT / 64; ++w) r += sh[w * K + k];
            v[k] = r;
        }
    __syncthreads();
}

// K maxima over the block at once, as block_sum_multi (valid in thread 0).
template <int NT, int K>
__device__ void block_max_multi(double (&v)[K], double* sh) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] = fmax(v[k], __shfl_down(v[k], off, 64));
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wid * K + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double r = sh[k];
            for (int w = 1; w < NT / 64; ++w) r = fmax(r, sh[w * K + k]);
            v[k] = r;
        }
    __syncthreads();
}

// ---- per-node tile reduction: one tile pass and one fold for every operation ----
// The plan (k_xbar, k_absdev, k_cost_rho_stats): a block per (tile, slot
// chunk), XB_CH slots per load batch, the tile's values stored with store_wt
// into `partial`; the last block to arrive (arrive_last) folds each node's
// tiles in a fixed order, so the result does not depend on which block is last.
// An operation type Op supplies what differs:
//   NS, NM          sums and maxima a slot carries (sums first: values 0..NS-1)
//   ENTRY           whether the pass reads a value per node entry (entry());
//                   the tile -> node lookup is compiled in only then
//   Loads, load()   one scenario's loads for the XB_CH slots of a batch
//   add()           its contribution to acc[k * XB_CH + c] / mx[k * XB_CH + c]
//   at()            where value k of (tile offset o, slot l) sits in `partial`
//   count(), store()  the node entry's write (count: the node's local scenarios,
//                   for the operations that store it)
#define XB_CH 4       // nonant slots per load batch
#define XB_SEQ_TILES 32   // a node of at most this many tiles is folded slot-parallel, in tile order
// ... and a node of at least this many slots, whatever its tile count (netdes:
// 1,470 slots over 40 tiles were 368 block reductions in a row, 1.1 ms, r06 s11)
#define XB_SEQ_SLOTS 64
#define XB_NODE_PAR 16    // from this many nodes a thread per node folds (fold_all)

struct TileMap { const int32_t *s0, *s1, *slot, *nlen, *out; };                  // per tile
struct NodeMap { int nnodes; const int32_t *tile_ptr, *off, *nlen, *tile_out; }; // per local node

// Tile t: the operation's values over the tile's scenarios for each slot of
// its node.  Slots in chunks of XB_CH, a scenario per thread and pass (256 per
// pass of a block): every load of a chunk is in flight at once; the chunk's
// sums share one block reduction, its maxima another.  Fixed order throughout.
// (ch, nch: this block takes slot chunks ch, ch + nch, ...; a tile's chunks are
// spread over nch blocks when the tiles alone are too few to fill the chip --
// C2 farmer cm=10: 4 tiles of 30 slots took 64 us in one block each)
template <class Op>
__device__ void tile_pass(const Op& op, const TileMap& T, const NodeMap& Nd, int t, int ch, int nch,
                          double* partial, double* sh) {
    constexpr int NS = Op::NS, NM = Op::NM;
    int e0 = 0;
    if constexpr (Op::ENTRY) {
        __shared__ int s_node;
        // the tile's node (its first entry): the one whose tile range holds t
        for (int v = threadIdx.x; v < Nd.nnodes; v += RED_NT)
            if (Nd.tile_ptr[v] <= t && t < Nd.tile_ptr[v + 1]) s_node = v;
        __syncthreads();
        e0 = Nd.off[s_node];
    }
    const int s0 = T.s0[t], s1 = T.s1[t], sl0 = T.slot[t], nl = T.nlen[t];
    const int out = T.out[t];
    for (int l0 = ch * XB_CH; l0 < nl; l0 += nch * XB_CH) {
        double acc[NS * XB_CH], mx[(NM ? NM : 1) * XB_CH], en[XB_CH];
#pragma unroll
        for (int k = 0; k < NS * XB_CH; ++k) acc[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NM * XB_CH; ++k) mx[k] = -INFINITY;
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) {
            en[c] = 0.0;
            if constexpr (Op::ENTRY) en[c] = op.entry(e0 + l0 + c, l0 + c < nl);
        }
        for (int g = s0; g < s1; g += RED_NT) {
            const int sc = g + (int)threadIdx.x;
            typename Op::Loads ld;
            op.load(ld, sc, sc < s1, sl0, l0, nl);
            op.add(ld, en, sc < s1, l0, nl, acc, mx);
        }
        block_sum_multi<RED_NT, NS * XB_CH>(acc, sh);
        if constexpr (NM > 0) block_max_multi<RED_NT, NM * XB_CH>(mx, sh);
        // (a guarded unrolled loop: with the bound in the loop condition acc
        // was indexed dynamically and lived in scratch, 80 B per lane)
        if (threadIdx.x == 0)
#pragma unroll
            for (int c = 0; c < XB_CH; ++c)
                if (l0 + c < nl) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) store_wt(&partial[op.at(k, out, nl, l0 + c)], acc[k * XB_CH + c]);
#pragma unroll
                    for (int k = 0; k < NM; ++k)
                        store_wt(&partial[op.at(NS + k, out, nl, l0 + c)], mx[k * XB_CH + c]);
                }
    }
}

// Entry (node, slot l): its tile partials in tile order -- sums added, maxima
// taken -- by one thread.
template <class Op>
__device__ __forceinline__ void fold_entry(const Op& op, int t0, int t1, int o0, int nl, int l, int e, double cnt,
                                           const double* partial) {
    constexpr int NS = Op::NS, NM = Op::NM;
    double r[NS + NM];
#pragma unroll
    for (int k = 0; k < NS + NM; ++k) r[k] = k < NS ? 0.0 : -INFINITY;
    for (int t = t0; t < t1; ++t) {
        // a node's tiles are consecutive with consecutive partial slots of 2*nl
        // (phbase/spbase tree layout), so the offset needs no per-tile load
        const int o = o0 + (t - t0) * 2 * nl;
#pragma unroll
        for (int k = 0; k < NS + NM; ++k) {
            const double p = load_wt(&partial[op.at(k, o, nl, l)]);
            r[k] = k < NS ? r[k] + p : fmax(r[k], p);
        }
    }
    op.store(e, r, cnt);
}

// All nodes' entries from the tile partials, in one of three fixed orders
// (reproducible run to run).  Many nodes (multistage trees: aircond 10x10x10
// has 111, mostly of one or a few tiles): one thread per node takes its slots
// and tiles in order -- the node-by-node loop with two barriers per node cost
// ~200 us there.  A few nodes (two-stage trees), node by node: a thread per
// slot adds the tiles in tile order (one pass, no block reduction per slot
// chunk -- C2's 30 slots of 4 tiles took eight), or, for many tiles of few
// slots, the tiles spread over the block, XB_CH slots at a time.
template <class Op>
__device__ void fold_all(const Op& op, const NodeMap& Nd, const double* partial, double* sh) {
    constexpr int NS = Op::NS, NM = Op::NM;
    if (Nd.nnodes >= XB_NODE_PAR) {
        for (int v = threadIdx.x; v < Nd.nnodes; v += RED_NT) {
            const int nl = Nd.nlen[v], t0 = Nd.tile_ptr[v], t1 = Nd.tile_ptr[v + 1];
            const int o0 = Nd.tile_out[t0], e0 = Nd.off[v];
            const double cnt = op.count(t0, t1);
            for (int l = 0; l < nl; ++l) fold_entry(op, t0, t1, o0, nl, l, e0 + l, cnt, partial);
        }
        __syncthreads();
        return;
    }
    for (int v = 0; v < Nd.nnodes; ++v) {
        const int nl = Nd.nlen[v], t0 = Nd.tile_ptr[v], t1 = Nd.tile_ptr[v + 1];
        const int o0 = Nd.tile_out[t0], e0 = Nd.off[v];
        // (a node's scenarios are contiguous and its tiles sorted by first scenario)
        const double cnt = op.count(t0, t1);
        if (t1 - t0 <= XB_SEQ_TILES || nl >= XB_SEQ_SLOTS) {
            for (int l = threadIdx.x; l < nl; l += RED_NT) fold_entry(op, t0, t1, o0, nl, l, e0 + l, cnt, partial);
            continue;
        }
        for (int l0 = 0; l0 < nl; l0 += XB_CH) {
            double acc[NS * XB_CH], mx[(NM ? NM : 1) * XB_CH];
#pragma unroll
            for (int k = 0; k < NS * XB_CH; ++k) acc[k] = 0.0;
#pragma unroll
            for (int k = 0; k < NM * XB_CH; ++k) mx[k] = -INFINITY;
            for (int t = t0 + (int)threadIdx.x; t < t1; t += RED_NT) {
                const int o = o0 + (t - t0) * 2 * nl;
#pragma unroll
                for (int c = 0; c < XB_CH; ++c)
                    if (l0 + c < nl) {
#pragma unroll
                        for (int k = 0; k < NS; ++k) acc[k * XB_CH + c] += load_wt(&partial[op.at(k, o, nl, l0 + c)]);
#pragma unroll
                        for (int k = 0; k < NM; ++k)
                            mx[k * XB_CH + c] =
                                fmax(mx[k * XB_CH + c], load_wt(&partial[op.at(NS + k, o, nl, l0 + c)]));
                    }
            }
            block_sum_multi<RED_NT, NS * XB_CH>(acc, sh);
            if constexpr (NM > 0) block_max_multi<RED_NT, NM * XB_CH>(mx, sh);
            if (threadIdx.x == 0)
#pragma unroll
                for (int c = 0; c < XB_CH; ++c)
                    if (l0 + c < nl) {
                        double r[NS + NM];
#pragma unroll
                        for (int k = 0; k < NS + NM; ++k) r[k] = k < NS ? acc[k * XB_CH + c] : mx[(k - NS) * XB_CH + c];
                        op.store(e0 + l0 + c, r, cnt);
                    }
        }
    }
}

// Compute_Xbar: sum pc*x and pc*x^2 per (node, slot); a tile's 2 nlen slots of
// `partial` hold [sums of pc*x | sums of pc*x^2], the node sums [NNS | NNS].
struct XbarOp {
    static constexpr int NS = 2, NM = 0;
    static constexpr bool ENTRY = false;
    int S, NNS;
    const int32_t* slot_col;
    const double *x, *pc;
    double* node_sums;
    struct Loads { double xv[XB_CH], pv[XB_CH]; };
    __device__ void load(Loads& L, int sc, bool live, int sl0, int l0, int nl) const {
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) {
            const int l = l0 + c;
            const bool ok = live && l < nl;
            L.xv[c] = ok ? x[ix(slot_col[sl0 + l], sc, S)] : 0.0;
            L.pv[c] = ok ? pc[ix(sl0 + l, sc, S)] : 0.0;
        }
    }
    __device__ void add(const Loads& L, const double (&)[XB_CH], bool, int, int, double (&acc)[2 * XB_CH],
                        double (&)[XB_CH]) const {
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) {
            const double v = L.pv[c] * L.xv[c];
            acc[c] += v;
            acc[XB_CH + c] += v * L.xv[c];
        }
    }
    __device__ int at(int k, int o, int nl, int l) const { return o + k * nl + l; }
    __device__ double count(int, int) const { return 0.0; }
    __device__ void store(int e, const double (&r)[2], double) const {
        node_sums[e] = r[0];
        node_sums[NNS + e] = r[1];
    }
};

// All nodes' x-bar sums from k_xbar's tile partials (k_xbar's last block, and
// every k_update_w_seg block on the from_tiles path)
__device__ void xbar_fold_all(int nnodes, const int32_t* node_tile_ptr, const int32_t* node_off,
                              const int32_t* node_nlen, const int32_t* tile_out, int NNS, const double* partial,
                              double* node_sums, double* sh) {
    fold_all(XbarOp{0, NNS, nullptr, nullptr, nullptr, node_sums},
             NodeMap{nnodes, node_tile_ptr, node_off, node_nlen, tile_out}, partial, sh);
}

// Compute_Xbar local part in ONE launch: one block per tile, the last block
// to finish folds the tile partials into the node sums (fixed order, so the
// result does not depend on which block is last).
// k_xbar's grid: the tiles, times slot-chunk blocks while the tiles are few
static unsigned xbar_grid(int ntiles, int NNS) {
    if (ntiles <= 0) return 0;
    const int chunks = (NNS + XB_CH - 1) / XB_CH;
    // (up to ~2,048 blocks: netdes' 40 tiles of 368 slot chunks ran 31 chunks in a
    // row per block at 512; a chunk's sums do not depend on which block takes it)
    const int nch = std::max(1, std::min(chunks, std::max(512, std::min(2048, 8 * chunks)) / ntiles));
    return (unsigned)(ntiles * nch);
}

__global__ __launch_bounds__(RED_NT) void k_xbar(
    int S, int ntiles, const int32_t* tile_s0, const int32_t* tile_s1, const int32_t* tile_slot,
    const int32_t* tile_nlen, const int32_t* tile_out, const int32_t* slot_col, const double* x,
    const double* pc, double* partial, int nnodes, const int32_t* node_tile_ptr, const int32_t* node_off,
    const int32_t* node_nlen, int NNS, double* node_sums, unsigned int* ticket, const int32_t* gate,
    const int32_t* prev_left, int finish) {
    __shared__ double sh[RED_NT / 64 * 2 * XB_CH];
    if (phx_lane::gated(gate)) return;          // phx_iterk: past the device-side stop
    // phx_iterk: lanes the previous solve left to the generic path travel in
    // the slot after the sums (all-reduced with them, tested by Update_W)
    if (prev_left && blockIdx.x == 0 && threadIdx.x == 0) node_sums[2 * NNS] = (double)*prev_left;
    // the grid is ntiles x nch (xbar_grid): block b takes tile b % ntiles, chunk b / ntiles
    const int nch = (int)gridDim.x / ntiles;
    const NodeMap Nd{nnodes, node_tile_ptr, node_off, node_nlen, tile_out};
    tile_pass(XbarOp{S, NNS, slot_col, x, pc, node_sums}, TileMap{tile_s0, tile_s1, tile_slot, tile_nlen, tile_out},
              Nd, (int)blockIdx.x % ntiles, (int)blockIdx.x / ntiles, nch, partial, sh);
    if (!finish) return;          // phx_iterk, one rank: every Update_W block folds the tiles itself
    if (!arrive_last(ticket, gridDim.x)) return;
    xbar_fold_all(nnodes, node_tile_ptr, node_off, node_nlen, tile_out, NNS, partial, node_sums, sh);
}

__global__ void k_zero(double* p, int64_t n, const int32_t* gate) {
    if (phx_lane::gated(gate)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = 0.0;
}

__global__ void k_update_w(int N, int S, const int32_t* slot_col, const double* x,
                           const double* xbar_node, const int32_t* xbar_idx,
                           const double* rho, const double* Win, double* W, int update, double* dsum) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double d = 0.0;
    for (int j = 0; j < N; ++j) {
        const int64_t o = ix(j, s, S);
        const double diff = x[ix(slot_col[j], s, S)] - xbar_node[xbar_idx[o]];
        if (update) W[o] = Win[o] + rho[o] * diff;
        d += fabs(diff);
    }
    dsum[s] = d;
}

// ---- phx_iterk: device-side loop control ----
// Progress word in mapped host memory, polled by the host (no event / copy).
using phx_lane::IterkProgress;     // mapped progress word (phx_lane.h)

struct IterkCtl {
    int32_t* ctl;              // device [4]: [0] stop flag (the gate of later kernels), [1] stop iteration
    const double* strag;       // all-reduced straggler count of the previous solve
    const double* stage;       // this iteration's node sums (all-reduced)
    double* node_sums;         // the caller's xbar/xsqbar buffer (published when the step proceeds)
    int n_publish;             // 2*NNS
    int iter;
    int do_conv;               // compute convergence_diff in the same launch (one rank)
    const double* conv_cnt;    // [R] element counts per emulated rank
    int R;
    double thresh;
    IterkProgress* prog;       // device alias of the mapped progress word
    // one rank, few tree nodes: k_xbar leaves its tile partials and every
    // Update_W block folds them into the node sums itself (in LDS), which
    // saves k_xbar's arrival and last-block pass
    int from_tiles;
    const double* tpart;
    const int32_t *ntp, *noff, *nnl, *tout;
    int nnodes;
};
#define UW_NODE_LDS 2048           // 2*NNS limit of the from_tiles path

using phx_lane::publish_progress;

// convergence_diff (phbase.py:330-343): mean over emulated ranks of the
// per-rank mean |x - xbar|, in the host's order; conv < thresh stops
// (phbase.py:914-926) before this iteration's solve.
// (k_small_xw sums in registers and calls conv_publish itself)
__device__ __forceinline__ void conv_publish(const IterkCtl& ic, double tot) {
    const double conv = tot / ic.R;
    const int done = conv < ic.thresh ? 1 : 0;
    if (done) {
        ic.ctl[1] = ic.iter;
        *(volatile int32_t*)ic.ctl = 1;
    }
    publish_progress(ic.prog, ic.iter, done, conv);
}
__device__ void conv_finish(const IterkCtl& ic, const double* seg) {
    double tot = 0.0;
    for (int r = 0; r < ic.R; ++r) {
        const double c = ic.conv_cnt[r];
        if (c > 0) tot += seg[r] / c;
    }
    conv_publish(ic, tot);
}
#define UW_SPT 1      // scenarios per thread (tiles of UW_SPT * RED_NT = 256 scenarios)
#define UW_CH 8       // nonant slots per load batch (C2: 30 slots in four batches, not eight)
// Update_W + convergence partials fused over segment tiles (tiles partition
// [0,S) and never straddle an emulated-rank segment): per scenario
//   W += rho (x_N - xbar), d = sum_j |x_N - xbar|
// and partial[t] = sum of d over tile t (fixed order: per-thread strided sum,
// then the block tree).  dsum may be null.
__global__ __launch_bounds__(RED_NT) void k_update_w_seg(int N, int S, const int32_t* slot_col,
                                                         const double* x, const double* xbar_node,
                                                         const int32_t* xbar_idx, const double* rho,
                                                         const double* Win, double* W, int update, double* dsum,
                                                         const int32_t* ts0, const int32_t* ts1,
                                                         double* partial, int nseg, const int32_t* seg_tile_ptr,
                                                         double* seg_sums, unsigned int* ticket, IterkCtl ic) {
    __shared__ double sh[RED_NT / 64 * 2 * XB_CH];
    __shared__ double s_nodes[UW_NODE_LDS];
    const int t = blockIdx.x;
    if (ic.ctl) {
        // phx_iterk: nothing past the stop; a previous solve that left lanes to
        // the generic path stops the pipeline here (the same decision on every
        // rank: the count was all-reduced with the node sums)
        if (*(volatile int32_t*)ic.ctl) return;
        if (*ic.strag > 0.5) {
            if (t == 0 && threadIdx.x == 0) {
                ic.ctl[0] = 2;
                ic.ctl[1] = ic.iter;
                publish_progress(ic.prog, ic.iter, 2, 0.0);
            }
            return;
        }
        if (ic.from_tiles) {
            xbar_fold_all(ic.nnodes, ic.ntp, ic.noff, ic.nnl, ic.tout, ic.n_publish / 2, ic.tpart, s_nodes, sh);
            __syncthreads();
            xbar_node = s_nodes;
        }
        // publish the node sums this iteration's W update and solve use
        if (t == 0)
            for (int e = threadIdx.x; e < ic.n_publish; e += RED_NT) ic.node_sums[e] = xbar_node[e];
    }
    // Every thread owns up to UW_SPT scenarios of the tile and the slots in
    // chunks of UW_CH: all loads of a chunk are issued before its arithmetic
    // and stores (W may alias W_in), so a thread waits for memory once per
    // chunk instead of once per (slot, scenario).
    const int s0 = ts0[t], s1 = ts1[t];
    double dsc[UW_SPT];
#pragma unroll
    for (int u = 0; u < UW_SPT; ++u) dsc[u] = 0.0;
    for (int j0 = 0; j0 < N; j0 += UW_CH) {
        double xv[UW_SPT][UW_CH], xb[UW_SPT][UW_CH], wv[UW_SPT][UW_CH], rv[UW_SPT][UW_CH];
        int32_t id[UW_SPT][UW_CH];
#pragma unroll
        for (int u = 0; u < UW_SPT; ++u) {
            const int sc = s0 + (int)threadIdx.x + u * RED_NT;
#pragma unroll
            for (int c = 0; c < UW_CH; ++c) {
                const int jj = j0 + c;
                const bool ok = sc < s1 && jj < N;
                const int64_t o = ok ? ix(jj, sc, S) : 0;
                xv[u][c] = ok ? x[ix(slot_col[jj], sc, S)] : 0.0;
                id[u][c] = ok ? xbar_idx[o] : 0;
                wv[u][c] = (ok && update) ? Win[o] : 0.0;
                rv[u][c] = (ok && update) ? rho[o] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < UW_SPT; ++u)
#pragma unroll
            for (int c = 0; c < UW_CH; ++c) xb[u][c] = xbar_node[id[u][c]];
#pragma unroll
        for (int u = 0; u < UW_SPT; ++u) {
            const int sc = s0 + (int)threadIdx.x + u * RED_NT;
#pragma unroll
            for (int c = 0; c < UW_CH; ++c) {
                const int jj = j0 + c;
                if (sc < s1 && jj < N) {
                    const double diff = xv[u][c] - xb[u][c];
                    if (update) W[ix(jj, sc, S)] = wv[u][c] + rv[u][c] * diff;
                    dsc[u] += fabs(diff);
                }
            }
        }
    }
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < UW_SPT; ++u) {
        const int sc = s0 + (int)threadIdx.x + u * RED_NT;
        if (sc < s1) {
            if (dsum) dsum[sc] = dsc[u];
            a += dsc[u];
        }
    }
    const double r = block_sum<RED_NT>(a, sh);
    if (threadIdx.x == 0) store_wt(&partial[t], r);
    // the last block folds the tile partials into the per-segment sums
    if (!arrive_last(ticket, gridDim.x)) return;
    for (int g = 0; g < nseg; ++g) {
        double b = 0.0;
        for (int k = seg_tile_ptr[g] + (int)threadIdx.x; k < seg_tile_ptr[g + 1]; k += RED_NT) b += load_wt(&partial[k]);
        const double rb = block_sum<RED_NT>(b, sh);
        if (threadIdx.x == 0) seg_sums[g] = rb;
    }
    if (threadIdx.x == 0 && ic.ctl && ic.do_conv) conv_finish(ic, seg_sums);
}

// Update_W + convergence partials for many nonant slots per scenario (netdes:
// 1,470): k_update_w_seg's tiles times chunks of uw2_chunk slots, one block each
// (flattened: block b = tile b / nch, chunk b % nch), instead of one block per
// tile whose threads walked every slot (1.9 ms on 40 CUs at netdes 10k, r06
// s11).  The per-block sums of |x - x-bar| are folded per segment by the last
// block, over its tiles and their chunks in order -- a fixed order, the one
// phx_update_w's host loop takes too.
#define UW2_MIN_N 16
static int uw2_chunk(int N) { return N >= 64 ? 32 : 8; }   // (C2's 30 slots: 4 chunks of 8)
__global__ __launch_bounds__(RED_NT) void k_update_w_seg2(int N, int S, int nch, int CH, const int32_t* slot_col,
                                                          const double* x, const double* xbar_node,
                                                          const int32_t* xbar_idx, const double* rho,
                                                          const double* Win, double* W, int update,
                                                          const int32_t* ts0, const int32_t* ts1, double* partial,
                                                          int nseg, const int32_t* seg_tile_ptr, double* seg_sums,
                                                          unsigned int* ticket, IterkCtl ic) {
    __shared__ double sh[RED_NT / 64];
    const int b = blockIdx.x, t = b / nch, ch = b - t * nch;
    if (ic.ctl) {
        if (*(volatile int32_t*)ic.ctl) return;
        if (*ic.strag > 0.5) {
            if (b == 0 && threadIdx.x == 0) {
                ic.ctl[0] = 2;
                ic.ctl[1] = ic.iter;
                publish_progress(ic.prog, ic.iter, 2, 0.0);
            }
            return;
        }
        if (b == 0)
            for (int e = threadIdx.x; e < ic.n_publish; e += RED_NT) ic.node_sums[e] = xbar_node[e];
    }
    const int s1 = ts1[t], sc = ts0[t] + (int)threadIdx.x;
    const bool live = sc < s1;
    const int j1 = min(N, (ch + 1) * CH);
    double dsc = 0.0;
    for (int j0 = ch * CH; j0 < j1; j0 += 8) {
        double xv[8], xb[8], wv[8], rv[8];
        int32_t id[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int jj = j0 + c;
            const bool ok = live && jj < j1;
            const int64_t o = ok ? ix(jj, sc, S) : 0;
            xv[c] = ok ? x[ix(slot_col[jj], sc, S)] : 0.0;
            id[c] = ok ? xbar_idx[o] : 0;
            wv[c] = (ok && update) ? Win[o] : 0.0;
            rv[c] = (ok && update) ? rho[o] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) xb[c] = xbar_node[id[c]];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int jj = j0 + c;
            if (live && jj < j1) {
                const double diff = xv[c] - xb[c];
                if (update) W[ix(jj, sc, S)] = wv[c] + rv[c] * diff;
                dsc += fabs(diff);
            }
        }
    }
    const double r = block_sum<RED_NT>(dsc, sh);
    if (threadIdx.x == 0) store_wt(&partial[b], r);
    if (!arrive_last(ticket, gridDim.x)) return;
    for (int g = 0; g < nseg; ++g) {
        double a = 0.0;
        const int k0 = seg_tile_ptr[g] * nch, k1 = seg_tile_ptr[g + 1] * nch;
        for (int k = k0 + (int)threadIdx.x; k < k1; k += RED_NT) a += load_wt(&partial[k]);
        const double rb = block_sum<RED_NT>(a, sh);
        if (threadIdx.x == 0) seg_sums[g] = rb;
    }
    if (threadIdx.x == 0 && ic.ctl && ic.do_conv) conv_finish(ic, seg_sums);
}

// ---- Compute_Xbar + Update_W + convergence_diff of a small batch in ONE block ----
// (S <= 1024 scenarios, one thread each: aircond 10x10x10's 1,000 scenarios over
// 111 nodes took k_xbar 8.6 + k_update_w_seg 9.3 us per PH iteration and the gap
// between them, r05).  Every load of a scenario is issued at entry; the node
// sums are segmented wavefront scans (the scenarios of a node are contiguous:
// for each slot the lanes of a wavefront form runs of equal node keys), each
// run's sum stored per (key, wavefront), and a thread per key adding its
// wavefronts in order -- a fixed order throughout.  phx_xbar / phx_update_w take
// the same path at these sizes (modes 1 / 2), so the host loop's x-bar, W and
// convergence sums are bit for bit the device loop's (mode 3).
#define SX_NT 1024
#define SX_NMAX 8          // nonant slots per scenario
#define SX_SEG 8           // emulated-rank segments
#define SX_WAVES (SX_NT / 64)
#define SX_LDS_MAX 65536  // bytes of dynamic LDS (small_xw_lds: NNS <= 237)
struct SmallXW {
    int mode;              // 1: x-bar sums; 2: W update + convergence sums; 3: both (phx_iterk, one rank)
    int S, N, NNS, nnodes;
    int32_t scol[SX_NMAX]; // the slots' columns, by value (no load before the x loads)
    const double* x;
    const double* pc;
    const int32_t* xbar_idx;
    const int32_t *node_tile_ptr, *node_off, *node_nlen, *tile_s0, *tile_s1;
    double* node_sums;     // out (modes 1, 3: [sum p x | sum p x^2]); in (mode 2)
    const double* rho;
    const double* Win;
    double* W;
    int update;
    double* dsum;
    int nseg;
    int seg_s0[SX_SEG], seg_s1[SX_SEG];
    double* seg_sums;
    const int32_t* prev_left;   // mode 3: the previous solve's leftover count (stops the pipeline)
};

// The runs of equal key in a wavefront (contiguous): the mask of the lanes that
// start a run (one shuffle, one ballot).  Lane l's run starts at the highest set
// bit at or below l, and l ends its run when l is 63 or bit l + 1 is set.
__device__ __forceinline__ unsigned long long run_starts(int key, int lane) {
    const int kp = __shfl_up(key, 1, 64);
    return __ballot(lane == 0 || kp != key);
}
__device__ __forceinline__ int run_start(unsigned long long starts, int lane) {
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    return 63 - __clzll(starts & upto);
}
// v of the DPP source lane (0 where the control names none)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_mov(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u & 0xffffffffull), CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROWMASK, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// inclusive scan of v over the runs (rs: the lane's run start); the sum of a run
// ends up in its last lane.  DPP steps, VALU only (a __shfl_up per step was two
// ds_bpermute round trips through the LDS crossbar, and 16 wavefronts x 12
// scans queued on one CU's LDS): row_shr 1, 2, 4, 8 inside each row of 16 lanes
// (lane then holds [max(row start, rs), lane]), then the last lane of the row
// before into rows 1 and 3 (row_bcast:15) and lane 31 into rows 2 and 3
// (row_bcast:31).  A source lane's value is added iff it lies in the lane's
// run (source >= rs, so the source's own run start is rs).  A fixed order.
__device__ __forceinline__ double run_scan(double v, int rs, int lane) {
    const int r = lane & 15;
    double u;
    u = dpp_mov<0x111, 0xf>(v);
    if (r >= 1 && lane - 1 >= rs) v += u;
    u = dpp_mov<0x112, 0xf>(v);
    if (r >= 2 && lane - 2 >= rs) v += u;
    u = dpp_mov<0x114, 0xf>(v);
    if (r >= 4 && lane - 4 >= rs) v += u;
    u = dpp_mov<0x118, 0xf>(v);
    if (r >= 8 && lane - 8 >= rs) v += u;
    u = dpp_mov<0x142, 0xa>(v);
    if (((lane >> 4) & 1) && (lane | 15) - 16 >= rs) v += u;
    u = dpp_mov<0x143, 0xc>(v);
    if (lane >= 32 && 31 >= rs) v += u;
    return v;
}

// dynamic LDS: [run sums 2 NNS x SX_WAVES | node sums 2 NNS | segment parts SX_SEG x SX_WAVES]
static size_t small_xw_lds(int NNS) {
    return sizeof(double) * ((size_t)2 * NNS * (SX_WAVES + 1) + SX_SEG * SX_WAVES);
}
__global__ __launch_bounds__(SX_NT) void k_small_xw(SmallXW a, IterkCtl ic) {
    extern __shared__ double sx_lds[];
    double* s_runs = sx_lds;
    double* s_nodes = sx_lds + (size_t)2 * a.NNS * SX_WAVES;
    double* s_seg = s_nodes + 2 * a.NNS;
    const int s = (int)threadIdx.x, lane = s & 63, wv = s >> 6;
    const bool live = s < a.S;
    const int S = a.S, N = a.N;
    // Every load issued at entry, before the gate and the previous solve's
    // count are known (loads have no effects; a gated launch drops them): the
    // scenario's x / keys / pc / W / rho, this thread's node (the node fold's
    // first v = s: its tile range, entries, first and last wavefront) and, in
    // thread 0, the emulated ranks' counts.  Loaded behind the gate and behind
    // each other they were ~6 dependent memory round trips of a ~17 us kernel
    // (aircond 10x10x10, r06 s27 trace).  The same values and arithmetic.
    double xv[SX_NMAX], pv[SX_NMAX], wvv[SX_NMAX], rv[SX_NMAX];
    int id[SX_NMAX];
#pragma unroll
    for (int j = 0; j < SX_NMAX; ++j) {
        const bool ok = live && j < N;
        const int64_t o = ok ? ix(j, s, S) : 0;
        xv[j] = ok ? a.x[ix(a.scol[j], s, S)] : 0.0;
        id[j] = ok ? a.xbar_idx[o] : -1 - s;
        pv[j] = (ok && a.mode != 2) ? a.pc[o] : 0.0;
        wvv[j] = (ok && a.mode != 1 && a.update) ? a.Win[o] : 0.0;
        rv[j] = (ok && a.mode != 1 && a.update) ? a.rho[o] : 0.0;
    }
    const bool own_node = a.mode != 2 && s < a.nnodes;
    int nd_t0 = 0, nd_t1 = 0, nd_nl = 0, nd_e0 = 0;
    if (own_node) {
        nd_t0 = a.node_tile_ptr[s];
        nd_t1 = a.node_tile_ptr[s + 1];
        nd_nl = a.node_nlen[s];
        nd_e0 = a.node_off[s];
    }
    double ccnt[SX_SEG];
    const bool cnt_pre = a.mode == 3 && s == 0 && ic.R <= SX_SEG;
#pragma unroll
    for (int r = 0; r < SX_SEG; ++r) ccnt[r] = (cnt_pre && r < ic.R) ? ic.conv_cnt[r] : 0.0;
    const int32_t prev_left = a.mode == 3 ? *a.prev_left : 0;   // (written by an earlier launch)
    if (a.mode == 3) {
        // phx_iterk: nothing past the stop; a previous solve that left lanes to
        // the generic path stops the pipeline here (k_update_w_seg's rule)
        if (*(volatile int32_t*)ic.ctl) return;
        if (prev_left > 0) {
            if (s == 0) {
                ic.ctl[0] = 2;
                ic.ctl[1] = ic.iter;
                publish_progress(ic.prog, ic.iter, 2, 0.0);
            }
            return;
        }
    }
    // the node's first and last wavefront (behind its tile range; in flight
    // while the scans below run)
    int nd_w0 = 0, nd_w1 = -1;
    if (own_node && nd_t1 > nd_t0) {
        nd_w0 = a.tile_s0[nd_t0] >> 6;
        nd_w1 = (a.tile_s1[nd_t1 - 1] - 1) >> 6;
    }
    const double* xbn = a.node_sums;
    if (a.mode != 2) {
        // runs of equal node key per slot: scan, the run's last lane keeps its sum
#pragma unroll
        for (int j = 0; j < SX_NMAX; ++j) {
            if (j >= N) break;
            const int key = id[j];
            const double v = pv[j] * xv[j];
            const unsigned long long st = run_starts(key, lane);
            const int rs = run_start(st, lane);
            const double r1 = run_scan(v, rs, lane);
            const double r2 = run_scan(v * xv[j], rs, lane);
            if (live && (lane == 63 || ((st >> (lane + 1)) & 1ull))) {
                s_runs[key * SX_WAVES + wv] = r1;
                s_runs[(a.NNS + key) * SX_WAVES + wv] = r2;
            }
        }
        __syncthreads();
        // a thread per (node, slot): the node's wavefronts in order
        for (int v = s; v < a.nnodes; v += SX_NT) {
            // (v = s: loaded at entry; further nodes -- more than SX_NT -- here)
            const bool first = v == s;
            const int t0 = first ? nd_t0 : a.node_tile_ptr[v], t1 = first ? nd_t1 : a.node_tile_ptr[v + 1];
            const int nl = first ? nd_nl : a.node_nlen[v], e0 = first ? nd_e0 : a.node_off[v];
            const int w0 = first ? nd_w0 : (t1 > t0 ? a.tile_s0[t0] >> 6 : 0);
            const int w1 = first ? nd_w1 : (t1 > t0 ? (a.tile_s1[t1 - 1] - 1) >> 6 : -1);
            for (int l = 0; l < nl; ++l) {
                const int e = e0 + l;
                // the wavefronts' run sums four at a time (one LDS round trip
                // per four), added for w0..w1 in order
                double s1 = 0.0, s2 = 0.0;
                for (int q = w0 & ~3; q <= w1; q += 4) {
                    double r1[4], r2[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        r1[u] = s_runs[e * SX_WAVES + q + u];
                        r2[u] = s_runs[(a.NNS + e) * SX_WAVES + q + u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (q + u >= w0 && q + u <= w1) {
                            s1 += r1[u];
                            s2 += r2[u];
                        }
                }
                s_nodes[e] = s1;
                s_nodes[a.NNS + e] = s2;
                a.node_sums[e] = s1;                  // mode 3: the staging buffer
                a.node_sums[a.NNS + e] = s2;
                if (a.mode == 3) {                    // published: this step proceeds
                    ic.node_sums[e] = s1;
                    ic.node_sums[a.NNS + e] = s2;
                }
            }
        }
        if (a.mode == 1) return;
        __syncthreads();
        xbn = s_nodes;
    }
    // Update_W (phbase.py:293-318) and |x - x-bar| per scenario, k_update_w_seg's arithmetic
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < SX_NMAX; ++j) {
        if (j >= N) break;
        if (live) {
            const double diff = xv[j] - xbn[id[j]];
            if (a.update) a.W[ix(j, s, S)] = wvv[j] + rv[j] * diff;
            d += fabs(diff);
        }
    }
    if (live && a.dsum) a.dsum[s] = d;
    // per-segment sums: each wavefront's part (wave_sum's fixed DPP order), then the wavefronts in order
    for (int g = 0; g < a.nseg; ++g) {
        const double v = phx_lane::wave_sum((live && s >= a.seg_s0[g] && s < a.seg_s1[g]) ? d : 0.0);
        if (lane == 0) s_seg[g * SX_WAVES + wv] = v;
    }
    __syncthreads();
    if (s < a.nseg) {
        double t = 0.0;
        for (int w = 0; w < SX_WAVES; ++w) t += s_seg[s * SX_WAVES + w];
        a.seg_sums[s] = t;
        s_seg[s * SX_WAVES] = t;
    }
    if (a.mode == 3) {
        __syncthreads();
        if (s == 0) {
            // conv_finish's sum over the emulated ranks in order, unrolled over
            // SX_SEG so that the counts stay in registers (a runtime-indexed
            // local array is scratch memory, written by every thread at entry)
            double tot = 0.0;
            if (cnt_pre) {
#pragma unroll
                for (int r = 0; r < SX_SEG; ++r)
                    if (r < ic.R && ccnt[r] > 0) tot += s_seg[r * SX_WAVES] / ccnt[r];
            } else {
                for (int r = 0; r < ic.R; ++r) {
                    const double c = ic.conv_cnt[r];
                    if (c > 0) tot += s_seg[r * SX_WAVES] / c;
                }
            }
            conv_publish(ic, tot);
        }
    }
}

// phx_iterk on several ranks: convergence_diff after the all-reduce of the
// per-emulated-rank sums
__global__ void k_conv(IterkCtl ic, const double* seg_sums) {
    if (*(volatile int32_t*)ic.ctl) return;
    conv_finish(ic, seg_sums);
}

// segmented sums of a [S] vector: tile t covers [s0,s1) of segment seg[t]
__global__ __launch_bounds__(RED_NT) void k_seg_partial(const double* v, const int32_t* ts0,
                                                        const int32_t* ts1, double* partial) {
    __shared__ double sh[RED_NT / 64];
    const int t = blockIdx.x;
    double a = 0.0;
    for (int s = ts0[t] + (int)threadIdx.x; s < ts1[t]; s += RED_NT) a += v[s];
    const double r = block_sum<RED_NT>(a, sh);
    if (threadIdx.x == 0) partial[t] = r;
}

// One block per segment (emulated rank): its tile partials, fixed order.
__global__ __launch_bounds__(RED_NT) void k_seg_finish(int nseg, const int32_t* seg_tile_ptr,
                                                       const double* partial, double* out) {
    __shared__ double sh[RED_NT / 64];
    const int g = blockIdx.x;
    if (g >= nseg) return;
    double a = 0.0;
    for (int t = seg_tile_ptr[g] + (int)threadIdx.x; t < seg_tile_ptr[g + 1]; t += RED_NT) a += partial[t];
    const double r = block_sum<RED_NT>(a, sh);
    if (threadIdx.x == 0) out[g] = r;
}

// ---- per-scenario scalar sums: one one-block loop, one part loop, two folds ----
// phx_expect, phx_rho_sums, phx_w_absdiff: up to EXPECT_ONE_BLOCK scenarios one
// 1,024-thread block (sums_one_block); above, nb blocks of EXP_NT threads over
// chunk scenarios each (sums_part: block b sums its contiguous chunk, fixed
// order) and a fold of the block partials.  One 1024-thread block walking 100k
// scenarios took 30-50 us (each thread a chain of ~100 dependent loads); this
// is two short launches.  A term type supplies K, the number of sums, and
// add(s, v), scenario s's contribution to v[K].
constexpr int EXPECT_ONE_BLOCK = 8192;
struct ExpectGrid { int nb, chunk; };
static ExpectGrid expect_grid(int S) {
    const int nb = std::min(256, (S + 1023) / 1024);
    return ExpectGrid{nb, (S + nb - 1) / nb};
}

template <class Term>
__device__ void sums_one_block(const Term& t, int S, double* out) {
    constexpr int K = Term::K;
    __shared__ double sh[1024 / 64 * K];
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int s = threadIdx.x; s < S; s += 1024) t.add(s, v);
    block_sum_multi<1024, K>(v, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = v[k];
}

#define EXP_NT 256
template <class Term>
__device__ void sums_part(const Term& t, int S, int chunk, double* part) {
    constexpr int K = Term::K;
    __shared__ double sh[EXP_NT / 64 * K];
    const int s0 = blockIdx.x * chunk, s1 = min(S, s0 + chunk);
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int s = s0 + (int)threadIdx.x; s < s1; s += EXP_NT) t.add(s, v);
    block_sum_multi<EXP_NT, K>(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) part[(int64_t)k * gridDim.x + blockIdx.x] = v[k];
}

// The two fold orders of the block partials part[K][nb].  k_expect_fold: a
// thread per sum adds them in block order (phx_expect; k_iter0_keep's last
// block reproduces it) ...
__global__ __launch_bounds__(64) void k_expect_fold(int nb, const double* part, double* out) {
    if (threadIdx.x < 3) {
        double r = 0.0;
        for (int b = 0; b < nb; ++b) r += part[(int64_t)threadIdx.x * nb + b];
        out[threadIdx.x] = r;
    }
}
// ... k_sums_fold: a wavefront per sum (64 K threads), lane l adds blocks l,
// l + 64, ... in order, then the lanes by shuffles (phx_rho_sums, phx_w_absdiff)
// -- one thread walking 98 partials in a row took 8.4 us at 100,000 scenarios,
// 18.7 us over 256 at a million.  The orders differ, so an entry keeps its own.
__global__ __launch_bounds__(128) void k_sums_fold(int nb, const double* part, double* out) {
    const int k = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    double r = 0.0;
    for (int b = lane; b < nb; b += 64) r += part[(int64_t)k * nb + b];
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    if (lane == 0) out[k] = r;
}

// phx_expect's term: p*obj, p, p*[optimal].  KEEP (phx_iterk adopting a
// deferred Iter0 solve) also copies the objective and status for the trivial
// bound's per-scenario outer bounds.
template <bool KEEP>
struct ExpectTerm {
    static constexpr int K = 3;
    static constexpr bool WAVE_FOLD = false;
    const double *prob, *obj;
    const int32_t* status;
    double* obj_keep;
    int32_t* status_keep;
    __device__ static void contrib(double p, double f, int32_t st, double (&v)[3]) {
        v[0] += p * f;
        v[1] += p;
        v[2] += (st == OPTIMAL) ? p : 0.0;
    }
    __device__ void add(int s, double (&v)[3]) const {
        const double p = prob[s], f = obj[s];
        const int32_t st = status[s];
        if (KEEP) {
            obj_keep[s] = f;
            status_keep[s] = st;
        }
        contrib(p, f, st, v);
    }
};

__global__ __launch_bounds__(1024) void k_expect(ExpectTerm<false> t, int S, double* out) {
    sums_one_block(t, S, out);
}
__global__ __launch_bounds__(EXP_NT) void k_expect_part(ExpectTerm<false> t, int S, int chunk, double* part) {
    sums_part(t, S, chunk, part);
}

// ---- adaptive rho: per-(node, slot) primal residuals, the norm-rho rule, rho sums ----
// phx_node_absdev, small batches (where k_small_xw takes Compute_Xbar): one
// block, a thread per scenario, every load issued at entry; k_small_xw's
// segmented wavefront scans over the runs of equal node key, a thread per node
// adding its wavefronts in order, thread 0 the total in entry order.
struct AbsdevSmall {
    int S, N, NNS, nnodes, per_slot;
    int32_t scol[SX_NMAX];
    const double *x, *xbar, *wt;
    const int32_t* key;
    const int32_t *node_tile_ptr, *node_off, *node_nlen, *tile_s0, *tile_s1;
    double* out;           // [NNS + 1]
};
// dynamic LDS: [run sums NNS x SX_WAVES | entry sums NNS]
static size_t absdev_small_lds(int NNS) { return sizeof(double) * (size_t)NNS * (SX_WAVES + 1); }
// (the pass itself: k_absdev_small, and k_absdev_small_rho of the device loop;
// returns the entry sums in LDS, valid in every thread)
__device__ __forceinline__ const double* absdev_small_pass(const AbsdevSmall& a, double* ad_lds) {
    double* s_runs = ad_lds;
    double* s_out = ad_lds + (size_t)a.NNS * SX_WAVES;
    const int s = (int)threadIdx.x, lane = s & 63, wv = s >> 6;
    const bool live = s < a.S;
    const int S = a.S, N = a.N;
    double tv[SX_NMAX];
    int id[SX_NMAX];
    const double ws = (live && !a.per_slot) ? a.wt[s] : 0.0;
#pragma unroll
    for (int j = 0; j < SX_NMAX; ++j) {
        const bool ok = live && j < N;
        const int64_t o = ok ? ix(j, s, S) : 0;
        id[j] = ok ? a.key[o] : -1 - s;
        const double xv = ok ? a.x[ix(a.scol[j], s, S)] : 0.0;
        const double xb = ok ? a.xbar[id[j]] : 0.0;
        const double w = ok ? (a.per_slot ? a.wt[o] : ws) : 0.0;
        tv[j] = w * fabs(xv - xb);
    }
    const bool own_node = s < a.nnodes;
    int nd_t0 = 0, nd_t1 = 0, nd_nl = 0, nd_e0 = 0;
    if (own_node) {
        nd_t0 = a.node_tile_ptr[s];
        nd_t1 = a.node_tile_ptr[s + 1];
        nd_nl = a.node_nlen[s];
        nd_e0 = a.node_off[s];
    }
    int nd_w0 = 0, nd_w1 = -1;
    if (own_node && nd_t1 > nd_t0) {
        nd_w0 = a.tile_s0[nd_t0] >> 6;
        nd_w1 = (a.tile_s1[nd_t1 - 1] - 1) >> 6;
    }
    for (int e = s; e < a.NNS; e += SX_NT) s_out[e] = 0.0;   // (entries of nodes absent locally)
#pragma unroll
    for (int j = 0; j < SX_NMAX; ++j) {
        if (j >= N) break;
        const int key = id[j];
        const unsigned long long st = run_starts(key, lane);
        const int rs = run_start(st, lane);
        const double r1 = run_scan(tv[j], rs, lane);
        if (live && (lane == 63 || ((st >> (lane + 1)) & 1ull))) s_runs[key * SX_WAVES + wv] = r1;
    }
    __syncthreads();
    for (int v = s; v < a.nnodes; v += SX_NT) {
        const bool first = v == s;
        const int t0 = first ? nd_t0 : a.node_tile_ptr[v], t1 = first ? nd_t1 : a.node_tile_ptr[v + 1];
        const int nl = first ? nd_nl : a.node_nlen[v], e0 = first ? nd_e0 : a.node_off[v];
        const int w0 = first ? nd_w0 : (t1 > t0 ? a.tile_s0[t0] >> 6 : 0);
        const int w1 = first ? nd_w1 : (t1 > t0 ? (a.tile_s1[t1 - 1] - 1) >> 6 : -1);
        for (int l = 0; l < nl; ++l) {
            double r = 0.0;
            for (int w = w0; w <= w1; ++w) r += s_runs[(e0 + l) * SX_WAVES + w];
            s_out[e0 + l] = r;
            a.out[e0 + l] = r;
        }
    }
    __syncthreads();
    if (s == 0) {
        double tot = 0.0;
        for (int e = 0; e < a.NNS; ++e) tot += s_out[e];
        a.out[a.NNS] = tot;
    }
    return s_out;
}
__global__ __launch_bounds__(SX_NT) void k_absdev_small(AbsdevSmall a) {
    extern __shared__ double ad_lds[];
    absdev_small_pass(a, ad_lds);
}

// phx_node_absdev above that: k_xbar's layout (tile_pass / fold_all) -- the
// tile's sums of wt |x - xbar| into its slot of `partial` (the first nlen of the
// 2 nlen the x-bar layout reserves per tile); the last block to arrive adds
// each node's tiles in tile order and then the entries in index order.
struct AbsdevOp {
    static constexpr int NS = 1, NM = 0;
    static constexpr bool ENTRY = true;
    int S, per_slot;
    const int32_t* slot_col;
    const double *x, *xbar, *wt;
    double* out;
    struct Loads { double xv[XB_CH], wv[XB_CH]; };
    __device__ double entry(int e, bool ok) const { return ok ? xbar[e] : 0.0; }
    __device__ void load(Loads& L, int sc, bool live, int sl0, int l0, int nl) const {
        const double ws = (live && !per_slot) ? wt[sc] : 0.0;
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) {
            const int l = l0 + c;
            const bool ok = live && l < nl;
            L.xv[c] = ok ? x[ix(slot_col[sl0 + l], sc, S)] : 0.0;
            L.wv[c] = ok ? (per_slot ? wt[ix(sl0 + l, sc, S)] : ws) : 0.0;
        }
    }
    __device__ void add(const Loads& L, const double (&xb)[XB_CH], bool, int, int, double (&acc)[XB_CH],
                        double (&)[XB_CH]) const {
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) acc[c] += L.wv[c] * fabs(L.xv[c] - xb[c]);
    }
    __device__ int at(int, int o, int, int l) const { return o + l; }
    __device__ double count(int, int) const { return 0.0; }
    __device__ void store(int e, const double (&r)[1], double) const { out[e] = r[0]; }
};

struct AbsdevTiles {
    int S, ntiles, nnodes, NNS, per_slot;
    const int32_t *tile_s0, *tile_s1, *tile_slot, *tile_nlen, *tile_out, *slot_col;
    const int32_t *node_tile_ptr, *node_off, *node_nlen;
    const double *x, *xbar, *wt;
    double *partial, *out;
    unsigned int* ticket;
};
// (the pass itself: k_absdev, and k_absdev_rho of the device loop; true in the
// last block, once every entry and the total are stored)
__device__ __forceinline__ bool absdev_tiles_pass(const AbsdevTiles& a, double* sh) {
    const AbsdevOp op{a.S, a.per_slot, a.slot_col, a.x, a.xbar, a.wt, a.out};
    const NodeMap Nd{a.nnodes, a.node_tile_ptr, a.node_off, a.node_nlen, a.tile_out};
    // the grid is ntiles x nch (xbar_grid): block b takes tile b % ntiles, chunk b / ntiles
    const int nch = (int)gridDim.x / a.ntiles;
    tile_pass(op, TileMap{a.tile_s0, a.tile_s1, a.tile_slot, a.tile_nlen, a.tile_out}, Nd,
              (int)blockIdx.x % a.ntiles, (int)blockIdx.x / a.ntiles, nch, a.partial, sh);
    if (!arrive_last(a.ticket, gridDim.x)) return false;
    fold_all(op, Nd, a.partial, sh);
    __syncthreads();
    // the total in entry order (entries of absent nodes: the zeros of the fill before this launch)
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int e = 0; e < a.NNS; ++e) tot += a.out[e];
        a.out[a.NNS] = tot;
    }
    return true;
}
__global__ __launch_bounds__(RED_NT) void k_absdev(AbsdevTiles a) {
    __shared__ double sh[RED_NT / 64 * XB_CH];
    absdev_tiles_pass(a, sh);
}

// The norm-rho rule (norm_rho_updater.py:98-104, :122-143), a thread per local
// (node, slot) entry: thread v * N + l takes slot l of local node v.  The
// node's last local scenario ends its last tile (the tiles of a node are
// sorted by first scenario, SPBase._create_communicators).
struct NormRhoRule {
    double tol, inc, dec, factor, cdec;
    int allow;
};
// where the rule finds its entries and leaves its results (log_row: the row of
// the device loop's action log, or null)
struct RhoRuleIO {
    int nnodes, N, S;
    const int32_t *node_tile_ptr, *node_off, *node_nlen, *tile_s1, *tile_slot;
    const double* xbar;
    double* prev;
    const double* rho;
    double* dual_out;
    int32_t *action_out, *log_row;
};
// thread idx = v * N + l: the operands of slot l of local node v (e < 0: none)
struct RhoRuleEntry { int e; double xb, prev, rho_rep; };
__device__ __forceinline__ RhoRuleEntry rho_rule_load(const RhoRuleIO& io, int64_t idx) {
    RhoRuleEntry r{-1, 0.0, 0.0, 0.0};
    const int v = (int)(idx / io.N), l = (int)(idx % io.N);
    if (v >= io.nnodes || l >= io.node_nlen[v]) return r;
    const int tl = io.node_tile_ptr[v + 1] - 1;
    r.e = io.node_off[v] + l;
    r.xb = io.xbar[r.e];
    r.prev = io.prev[r.e];
    r.rho_rep = io.rho[ix(io.tile_slot[tl] + l, io.tile_s1[tl] - 1, io.S)];
    return r;
}
__device__ __forceinline__ void rho_rule_apply(const RhoRuleIO& io, const NormRhoRule& o, const RhoRuleEntry& r,
                                               double p) {
    const double d = r.rho_rep * fabs(r.xb - r.prev);
    int act = 0;
    if (p > o.factor * d && p > o.tol) {
        act = 1;
    } else if (d > o.factor * p && d > o.tol) {
        if (o.allow) act = 2;
    } else if (p < o.tol && d < o.tol) {
        act = 3;
    }
    io.action_out[r.e] = act;
    if (io.log_row) io.log_row[r.e] = act;
    if (io.dual_out) io.dual_out[r.e] = d;
    io.prev[r.e] = r.xb;
}
__global__ void k_norm_rho_rule(RhoRuleIO io, NormRhoRule o, const double* primal) {
    const RhoRuleEntry r = rho_rule_load(io, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (r.e >= 0) rho_rule_apply(io, o, r, primal[r.e]);
}

// rho[j][s] scaled by the action of its (node, slot) entry: IEEE multiply /
// divide (:135, :139, :142 -- not a multiplication by a reciprocal)
__device__ __forceinline__ void rho_scale_at(int64_t o, int64_t tot, const int32_t* xbar_idx, const int32_t* action,
                                             double inc, double dec, double cdec, double* rho) {
    if (o >= tot) return;
    const int act = action[xbar_idx[o]];
    if (act == 0) return;
    const double r = rho[o];
    rho[o] = act == 1 ? r * inc : (act == 2 ? r / dec : r / cdec);
}
__global__ void k_norm_rho_scale(int64_t tot, const int32_t* xbar_idx, const int32_t* action, double inc,
                                 double dec, double cdec, double* rho) {
    rho_scale_at((int64_t)blockIdx.x * blockDim.x + threadIdx.x, tot, xbar_idx, action, inc, dec, cdec, rho);
}

// ---- the update inside the device loop (phx_iterk_norm_rho) ----
// The reference's miditer sits between convergence_diff and the stop test
// (phbase.py:914-926), so the update of iteration k runs while the loop
// proceeds AND at the iteration that converged (ctl[0] == 1, ctl[1] == k); not
// at a straggler stop (ctl[0] == 2: that iteration is enqueued again once the
// leftovers are finished) and not past a stop (the padded iterations).  ctl is
// written by launches before these (Update_W / k_conv of the same iteration),
// so every block of a launch takes the same decision.
struct RhoGate { const int32_t* ctl; int iter; };
__device__ __forceinline__ bool rho_gated(const RhoGate& g) {
    const volatile int32_t* c = g.ctl;
    const int32_t f = c[0];
    return f != 0 && !(f == 1 && c[1] == g.iter);
}

// The first miditer of a run: x-bar_k into the snapshot, nothing else.
__global__ void k_rho_snapshot(RhoGate g, int NNS, const double* xbar, double* prev) {
    if (rho_gated(g)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < NNS) prev[e] = xbar[e];
}

// Entries of nodes absent locally (several ranks): residual 0 before the pass,
// action 0 and dual 0 for the rule -- phx_node_absdev's and phx_norm_rho's fills.
__global__ void k_rho_clear(RhoGate g, int NNS, double* primal, double* dual, int32_t* action, int32_t* log_row) {
    if (rho_gated(g)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > NNS) return;
    primal[e] = 0.0;
    if (e == NNS) return;
    action[e] = 0;
    if (log_row) log_row[e] = 0;
    if (dual) dual[e] = 0.0;
}

// phx_node_absdev's pass under the gate.  rule (one rank: the residuals are
// final without an all-reduce): the block that holds every entry -- the one
// block of the small path, the last block of the tiled one, which folded them
// -- evaluates the rule before it leaves, a thread per (node, slot) as
// k_norm_rho_rule.  That launch was three threads behind a chain of five
// dependent loads; here the small path issues the rule's loads with the pass's
// own at entry (x-bar, the snapshot and rho are final before this launch: rho
// is scaled by the launch after it, so rho_rep is read before any scale).
__global__ __launch_bounds__(SX_NT) void k_absdev_small_rho(AbsdevSmall a, RhoGate g, int rule, RhoRuleIO io,
                                                            NormRhoRule o) {
    extern __shared__ double ad_lds[];
    RhoRuleEntry pre{-1, 0.0, 0.0, 0.0};
    const int64_t nent = rule ? (int64_t)io.nnodes * io.N : 0;
    if ((int64_t)threadIdx.x < nent) pre = rho_rule_load(io, threadIdx.x);
    if (rho_gated(g)) return;
    const double* s_out = absdev_small_pass(a, ad_lds);
    for (int64_t idx = threadIdx.x; idx < nent; idx += SX_NT) {
        const RhoRuleEntry r = idx == (int64_t)threadIdx.x ? pre : rho_rule_load(io, idx);
        if (r.e >= 0) rho_rule_apply(io, o, r, s_out[r.e]);
    }
}
__global__ __launch_bounds__(RED_NT) void k_absdev_rho(AbsdevTiles a, RhoGate g, int rule, RhoRuleIO io,
                                                       NormRhoRule o) {
    __shared__ double sh[RED_NT / 64 * XB_CH];
    if (rho_gated(g)) return;
    if (!absdev_tiles_pass(a, sh) || !rule) return;
    // (the entries were stored by this block's threads before the pass's barrier)
    for (int64_t idx = threadIdx.x; idx < (int64_t)io.nnodes * io.N; idx += RED_NT) {
        const RhoRuleEntry r = rho_rule_load(io, idx);
        if (r.e >= 0) rho_rule_apply(io, o, r, a.out[r.e]);
    }
}
// several ranks: the rule behind the all-reduce of the residuals
__global__ void k_norm_rho_rule_gated(RhoGate g, RhoRuleIO io, NormRhoRule o, const double* primal) {
    if (rho_gated(g)) return;
    const RhoRuleEntry r = rho_rule_load(io, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (r.e >= 0) rho_rule_apply(io, o, r, primal[r.e]);
}
__global__ void k_norm_rho_scale_gated(RhoGate g, int64_t tot, const int32_t* xbar_idx, const int32_t* action,
                                       double inc, double dec, double cdec, double* rho) {
    if (rho_gated(g)) return;
    rho_scale_at((int64_t)blockIdx.x * blockDim.x + threadIdx.x, tot, xbar_idx, action, inc, dec, cdec, rho);
}

// phx_rho_sums: scenario s's terms, slots in order (one block up to
// EXPECT_ONE_BLOCK scenarios; above, block chunks and k_sums_fold)
struct RhoTerm {
    static constexpr int K = 2;
    static constexpr bool WAVE_FOLD = true;
    int N, S;
    const double *rho, *prob, *xb, *xp;
    const int32_t* idx;
    __device__ void add(int s, double (&v)[2]) const {
        double r = 0.0, d = 0.0;
        for (int j = 0; j < N; ++j) {
            const int64_t o = ix(j, s, S);
            const double rv = rho[o];
            r += rv;
            if (xp) {
                const int i = idx[o];
                d += rv * fabs(xb[i] - xp[i]);
            }
        }
        v[0] += prob[s] * r;
        v[1] += d;
    }
};
__global__ __launch_bounds__(1024) void k_rho_sums(RhoTerm t, int S, double* out) { sums_one_block(t, S, out); }
__global__ __launch_bounds__(EXP_NT) void k_rho_sums_part(RhoTerm t, int S, int chunk, double* part) {
    sums_part(t, S, chunk, part);
}

// ---- cost-proportional rho: candidate statistics, the order statistic, |W - W_prev| ----
// the scenario-dependent denominator: one scalar per scenario over both forms
// and every nonant slot (find_rho.py:189 np.max((w_denom, prox_denom)))
__global__ void k_cost_rho_denom(int N, int S, const int32_t* slot_col, const double* x, const double* xbar,
                                 const int32_t* idx, double* scen_denom) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double d = 0.0;
    for (int j = 0; j < N; ++j) {
        const double diff = x[ix(slot_col[j], s, S)] - xbar[idx[ix(j, s, S)]];
        const double sq = diff * diff;
        d = fmax(d, fmax(fabs(diff), 2.0 * sq));
    }
    scen_denom[s] = d;
}

// entries of nodes absent locally: 0, 0, -inf, -inf
__global__ void k_cost_rho_fill(int NNS, double* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 4 * NNS) out[t] = t < 2 * NNS ? 0.0 : -INFINITY;
}

__device__ __forceinline__ double cost_rho_term(double c, double d) {
    return d == 0.0 ? INFINITY : fabs(c) / d;
}

// k_absdev's layout (tile_pass / fold_all).  `partial` is [2 * npart]: the
// tile's sums in the first nlen of its 2 nlen x-bar slots, its max and -min in
// the 2 nlen of the second half.  A node entry: the sum, the node's local
// scenario count, the max and -min over its tiles.
struct CostRhoOp {
    static constexpr int NS = 1, NM = 2;
    static constexpr bool ENTRY = true;
    int S, npart, NNS;
    const int32_t *tile_s0, *tile_s1;
    const double *cost, *denom_node, *scen_denom;
    double* out;
    struct Loads { double cv[XB_CH], ds; };
    __device__ double entry(int e, bool ok) const { return (denom_node && ok) ? denom_node[e] : 0.0; }
    __device__ void load(Loads& L, int sc, bool live, int sl0, int l0, int nl) const {
        L.ds = (live && !denom_node) ? scen_denom[sc] : 0.0;
#pragma unroll
        for (int c = 0; c < XB_CH; ++c) L.cv[c] = (live && l0 + c < nl) ? cost[ix(sl0 + l0 + c, sc, S)] : 0.0;
    }
    __device__ void add(const Loads& L, const double (&dn)[XB_CH], bool live, int l0, int nl, double (&acc)[XB_CH],
                        double (&mx)[2 * XB_CH]) const {
#pragma unroll
        for (int c = 0; c < XB_CH; ++c)
            if (live && l0 + c < nl) {
                const double r = cost_rho_term(L.cv[c], denom_node ? dn[c] : L.ds);
                acc[c] += r;
                mx[c] = fmax(mx[c], r);
                mx[XB_CH + c] = fmax(mx[XB_CH + c], -r);
            }
    }
    __device__ int at(int k, int o, int nl, int l) const { return k == 0 ? o + l : npart + o + (k - 1) * nl + l; }
    // (a node's scenarios are contiguous and its tiles sorted by first scenario)
    __device__ double count(int t0, int t1) const { return (double)(tile_s1[t1 - 1] - tile_s0[t0]); }
    __device__ void store(int e, const double (&r)[3], double cnt) const {
        out[e] = r[0];
        out[NNS + e] = cnt;
        out[2 * NNS + e] = r[1];
        out[3 * NNS + e] = r[2];
    }
};

__global__ __launch_bounds__(RED_NT) void k_cost_rho_stats(
    int S, int ntiles, int npart, const int32_t* tile_s0, const int32_t* tile_s1, const int32_t* tile_slot,
    const int32_t* tile_nlen, const int32_t* tile_out, const double* cost, const double* denom_node,
    const double* scen_denom, double* partial, int nnodes, const int32_t* node_tile_ptr, const int32_t* node_off,
    const int32_t* node_nlen, int NNS, double* out, unsigned int* ticket) {
    __shared__ double sh[RED_NT / 64 * 2 * XB_CH];
    const CostRhoOp op{S, npart, NNS, tile_s0, tile_s1, cost, denom_node, scen_denom, out};
    const NodeMap Nd{nnodes, node_tile_ptr, node_off, node_nlen, tile_out};
    const int nch = (int)gridDim.x / ntiles;
    tile_pass(op, TileMap{tile_s0, tile_s1, tile_slot, tile_nlen, tile_out}, Nd, (int)blockIdx.x % ntiles,
              (int)blockIdx.x / ntiles, nch, partial, sh);
    if (!arrive_last(ticket, gridDim.x)) return;
    fold_all(op, Nd, partial, sh);
}

// Find_Rho._order_stat (find_rho.py:150-168) per (node, slot) entry, with its association
__global__ void k_cost_rho_rule(int NNS, double alpha, const double* stats, double* rho_node, int32_t* kept) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NNS) return;
    const double cnt = stats[NNS + e];
    const double mean = stats[e] / cnt, hi = stats[2 * NNS + e], lo = -stats[3 * NNS + e];
    double r;
    if (alpha == 0.5) r = mean;
    else if (alpha < 0.5) r = lo + alpha * 2 * (mean - lo);
    else r = (2 * mean - hi) + alpha * 2 * (hi - mean);
    rho_node[e] = r;
    kept[e] = (cnt > 0.0 && isfinite(r)) ? 0 : 1;
}

__global__ void k_cost_rho_bcast(int64_t tot, const int32_t* xbar_idx, const double* rho_node,
                                 const int32_t* kept, double* rho) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= tot) return;
    const int e = xbar_idx[o];
    if (kept[e] == 0) rho[o] = rho_node[e];
}

// phx_w_absdiff: scenario s's terms, slots in order; W_prev takes W (one block
// up to EXPECT_ONE_BLOCK scenarios, block chunks and k_sums_fold above, as
// phx_rho_sums)
struct WAbsdiffTerm {
    static constexpr int K = 1;
    static constexpr bool WAVE_FOLD = true;
    int N, S;
    const double* W;
    double* Wp;
    __device__ void add(int s, double (&v)[1]) const {
        double d = 0.0;
        for (int j = 0; j < N; ++j) {
            const int64_t o = ix(j, s, S);
            const double w = W[o];
            d += fabs(w - Wp[o]);
            Wp[o] = w;
        }
        v[0] += d;
    }
};
__global__ __launch_bounds__(1024) void k_w_absdiff(WAbsdiffTerm t, int S, double* out) { sums_one_block(t, S, out); }
__global__ __launch_bounds__(EXP_NT) void k_w_absdiff_part(WAbsdiffTerm t, int S, int chunk, double* part) {
    sums_part(t, S, chunk, part);
}

// Iter0's bookkeeping in one launch (phx_iterk adopting a deferred Iter0
// solve, S > EXPECT_ONE_BLOCK): its objectives and statuses copied for the trivial bound's
// per-scenario outer bounds, and phx_expect's three sums -- the same chunks and
// block sums as k_expect_part, and the last block to arrive adds the block
// partials in block order as k_expect_fold does, so the sums are phx_expect's
// bit for bit.  (Two copies and two expectation kernels were four dispatches,
// each ~5-15 us of solve-stream time with its gap.)
__global__ __launch_bounds__(EXP_NT) void k_iter0_keep(int S, int chunk, const double* prob, const double* obj,
                                                     const int32_t* status, double* obj_keep,
                                                     int32_t* status_keep, double* part, unsigned int* ticket,
                                                     double* out) {
    __shared__ double sh[EXP_NT / 64 * 3];
    __shared__ double pl[3 * 256];        // the last block's copy of the partials (nb <= 256)
    __shared__ bool last;
    const int s0 = blockIdx.x * chunk, s1 = min(S, s0 + chunk);
    double v[3] = {0.0, 0.0, 0.0};
    // (a thread's scenarios four at a time, every load of the four issued
    // before their stores and adds -- one memory round trip per four instead
    // of per scenario; the adds keep the scenario order)
    for (int s = s0 + (int)threadIdx.x; s < s1; s += 4 * EXP_NT) {
        double p[4], f[4];
        int32_t st[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int su = s + u * EXP_NT;
            const bool ok = su < s1;
            p[u] = ok ? prob[su] : 0.0;
            f[u] = ok ? obj[su] : 0.0;
            st[u] = ok ? status[su] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int su = s + u * EXP_NT;
            if (su < s1) {
                obj_keep[su] = f[u];
                status_keep[su] = st[u];
                ExpectTerm<true>::contrib(p[u], f[u], st[u], v);
            }
        }
    }
    block_sum_multi<EXP_NT, 3>(v, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; ++k) part[(int64_t)k * gridDim.x + blockIdx.x] = v[k];
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the partials into LDS in one round of loads (a thread per block), then
    // added in block order by three threads, as k_expect_fold does
    const int nb = (int)gridDim.x;
    for (int e = threadIdx.x; e < 3 * nb; e += EXP_NT) {
        const int k = e / nb, b = e - k * nb;
        pl[k * 256 + b] = __hip_atomic_load(&part[(int64_t)k * nb + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* pk = pl + threadIdx.x * 256;
        double r = 0.0;
        for (int b = 0; b < nb; ++b) r += pk[b];
        out[threadIdx.x] = r;
    }
    if (threadIdx.x == 0) *ticket = 0u;       // reusable
}

// k_iter0_keep for S <= EXPECT_ONE_BLOCK (phx_expect's one-block k_expect): k_expect's
// loop and block sums with the storing term, so the sums are k_expect's bit for bit.
// (aircond 1,000: two copy dispatches and k_expect were ~5 us each, r06 s40)
__global__ __launch_bounds__(1024) void k_iter0_keep1(ExpectTerm<true> t, int S, double* out) {
    sums_one_block(t, S, out);
}
