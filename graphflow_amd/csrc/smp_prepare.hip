// smp_prepare.hip -- a batch of molecules onto the device: the handle's pool of device blocks, the page-locked allocator of the host tables, the
// kernels that build the rows-sized level tables, gf_smp_prepare as a sequence of steps.  The host side of the preparation is smp_prep.cpp.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "smp_internal.h"

namespace gf {
// page-locked host memory for the per-batch tables (smp_prep.h: table_alloc): their uploads then run on the DMA engines beside
// the step that is executing, instead of blit kernels queued behind its compute kernels.  16-byte header: how it was obtained.
void *pinned_table_alloc(size_t bytes) {
    void *p = nullptr;
    const size_t total = bytes + 16;
    unsigned kind = 1;
    // (portable: the preparation's worker threads never call hipSetDevice, and a table pinned against device 0 only would be
    //  pageable memory to the uploads of every other rank's device)
    if (hipHostMalloc(&p, total, hipHostMallocPortable) != hipSuccess) p = nullptr;
    if (!p) {
        (void)hipGetLastError();
        p = std::malloc(total);
        kind = 0;
        if (!p) return nullptr;
    }
    *static_cast<unsigned *>(p) = kind;
    return static_cast<char *>(p) + 16;
}
void pinned_table_free(void *q) {
    if (!q) return;
    void *p = static_cast<char *>(q) - 16;
    if (*static_cast<unsigned *>(p) == 1)
        (void)hipHostFree(p);
    else
        std::free(p);
}

gf_status upload_bytes(gf_smp *s, void **dst, const void *src, size_t elem, size_t count) {
    *dst = nullptr;
    const size_t bytes = elem * (count ? count : 1);
    // best fit among the idle blocks of the pool (no block more than twice the request: keeps big blocks for big buffers)
    int best = -1;
    for (size_t i = 0; i < s->pool.size(); ++i) {
        const gf_smp::Block &b = s->pool[i];
        if (!b.used && b.bytes >= bytes && b.bytes <= 2 * bytes + 4096 && (best < 0 || b.bytes < s->pool[best].bytes)) best = (int)i;
    }
    void *p = nullptr;
    if (best >= 0) {
        s->pool[best].used = true;
        s->pool[best].idle = 0;
        p = s->pool[best].p;
    } else {
        const size_t cap = bytes + bytes / 8 + 256;  // slack: the next batch is about, not exactly, this size
        hipError_t e = hipMalloc(&p, cap);
        if (e != hipSuccess) return fail(s->ctx, GF_ERR_NOMEM, "smp: hipMalloc(%zu) failed: %s", cap, hipGetErrorString(e));
        gf_smp::Block b = {p, cap, true, 0};
        s->pool.push_back(b);
    }
    if (src && count)
        GF_HIP_TRY(s->ctx, hipMemcpyAsync(p, src, elem * count, hipMemcpyHostToDevice, s->upload ? s->upload : s->ctx->stream));
    else if (gf::poison_buffers()) {  // GF_POISON=1 (debug): a buffer handed out without contents is filled with NaN bit patterns, so a
        hipStream_t st = s->upload ? s->upload : s->ctx->stream;                    // read-before-write shows
        GF_HIP_TRY(s->ctx, hipMemsetAsync(p, 0xff, bytes, st));
        // (finished before anything else is launched: buffers are also taken from the pool in the middle of a pass -- the promoted
        //  stack of the op-by-op levels -- where the upload stream is not ordered against the pass)
        GF_HIP_TRY(s->ctx, hipStreamSynchronize(st));
    }
    *dst = p;
    return GF_OK;
}
gf_status ensure_P(gf_smp *s) { return s->P ? GF_OK : upload(s, &s->P, nullptr, s->P_count); }

// End of a batch: its buffers go back to the pool (blocks idle for three batches in a row are returned to the device).
// the handle's buffers were last touched by the launches before this mark
void mark_used(gf_smp *s) {
    if (s->ev_last && hipEventRecord(s->ev_last, s->ctx->stream) == hipSuccess) s->used = true;
}

void release(gf_smp *s) {
    if (s->ctx) {
        // wait for this handle's own work only: another handle of the context may be in the middle of its step
        if (s->ev_last) {
            if (s->used) (void)hipEventSynchronize(s->ev_last);
        } else {
            (void)hipStreamSynchronize(s->ctx->stream);
        }
        s->used = false;
    }
    std::vector<gf_smp::Block> keep;
    for (gf_smp::Block &b : s->pool) {
        if (!b.used && ++b.idle >= 3) {
            (void)hipFree(b.p);
            continue;
        }
        b.used = false;
        keep.push_back(b);
    }
    s->pool.swap(keep);
    static_cast<gf_smp_batch &>(*s) = gf_smp_batch();   // every pointer into those blocks and everything derived from the batch
}

void release_pool(gf_smp *s) {
    for (gf_smp::Block &b : s->pool) (void)hipFree(b.p);
    s->pool.clear();
}

namespace {
// rowscale[row] = (tot, tr) of the row's node (the per-row factors of the level's block products), from the per-node pairs
__global__ void expand_rowscale(float2 *__restrict__ rowscale, const float2 *__restrict__ node_scale, const int *__restrict__ node_s,
                                const long long *__restrict__ node_row) {
    const int n = blockIdx.x, s = node_s[n];
    const long long r0 = node_row[n];
    const float2 v = node_scale[n];
    for (int i = threadIdx.x; i < s * s; i += blockDim.x) rowscale[r0 + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// Level tables on the device (round 3; BatchLayout::device_tables).  What gfsmp::build_batch writes per node in its phase B --
// the reduced adjacency (SMP_omega.h:556-581: 1 on the diagonal and adj[v1][v2] elsewhere, or the Coulomb entries), its gated row
// sums and (tot, tr), the selection maps pi (:461-474) -- and per consumer entry in phase D (the inverse maps) are rows-sized:
// 2.2 of the 6.2 ms of host graph preparation on 32 threads (8 of 14 ms on 8) and 17 MB of the upload per 1024 molecules.  The
// kernels below build them from the receptive fields (sum-s ints per level), the pair tables and the molecules' adjacency
// matrices, with the host's summation orders (bit-identical tables: tests/test_smp_gpu.py::test_device_level_tables...).
// Workgroup per node; wave w builds the maps of the neighbours a = w, w + 4, ...
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void build_level_rows(const int *__restrict__ node_s, const int *__restrict__ node_mol,
                                                        const long long *__restrict__ node_row, const long long *__restrict__ node_pair,
                                                        const int *__restrict__ field, const int *__restrict__ prev_field,
                                                        const long long *__restrict__ pair_src_pair, const int *__restrict__ pair_src_s,
                                                        const int *__restrict__ mol_nv, const long long *__restrict__ mol_adj_off,
                                                        const int *__restrict__ mol_adj, const double *__restrict__ mol_coul,
                                                        float *__restrict__ adj, float *__restrict__ rsum, float *__restrict__ node_scale,
                                                        short *__restrict__ pi, int *__restrict__ node_present, int vmax) {
    extern __shared__ int lr_smem[];
    const int n = blockIdx.x, s = node_s[n], m = node_mol[n], V = mol_nv[m];
    const long long r0 = node_row[n], p0 = node_pair[n];
    int *f = lr_smem;                                             // [s] the node's field
    float *rs = reinterpret_cast<float *>(lr_smem + s);           // [s] gated row sums
    float *dg = rs + s;                                           // [s] gated diagonal
    short *pos = reinterpret_cast<short *>(dg + s);               // [4][vmax] position inside the source's field, -1 outside
    const int *madj = mol_adj + mol_adj_off[m];
    const double *mc = mol_coul ? mol_coul + mol_adj_off[m] : nullptr;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < s; i += blockDim.x) f[i] = field[p0 + i];
    for (int i = tid; i < 4 * vmax; i += blockDim.x) pos[i] = -1;
    __syncthreads();
    auto entry = [&](int i, int j) {
        return mc ? (float)mc[(size_t)f[i] * V + f[j]] : ((f[i] == f[j]) ? 1.f : (float)madj[(size_t)f[i] * V + f[j]]);
    };
    for (int idx = tid; idx < s * s; idx += blockDim.x) adj[r0 + idx] = entry(idx / s, idx % s);
    for (int i = tid; i < s; i += blockDim.x) {  // (entries with A <= 0 are skipped: RisiContraction_18.h:90; j in order, as the host sums)
        float acc = 0.f;
        for (int j = 0; j < s; ++j) {
            const float av = entry(i, j);
            if (av > 0.f) acc += av;
        }
        rs[i] = acc;
        rsum[p0 + i] = acc;
        const float d = entry(i, i);
        dg[i] = d > 0.f ? d : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f, tr = 0.f;
        for (int i = 0; i < s; ++i) {
            tot += rs[i];
            tr += dg[i];
        }
        node_scale[2 * (size_t)n] = tot;
        node_scale[2 * (size_t)n + 1] = tr;
    }
    short *mypos = pos + wave * vmax;
    unsigned cnt = 0;
    for (int a0 = 0; a0 < s; a0 += 4) {
        const int a = a0 + wave;
        const int *wf = nullptr;
        int sw = 0;
        if (a < s) {
            wf = prev_field + pair_src_pair[p0 + a];
            sw = pair_src_s[p0 + a];
            for (int k = lane; k < sw; k += 64) mypos[wf[k]] = (short)k;
        }
        __syncthreads();
        if (a < s)
            for (int p = lane; p < s; p += 64) {
                const short k = mypos[f[p]];
                pi[r0 + (long long)a * s + p] = k;
                cnt += k >= 0;
            }
        __syncthreads();
        if (a < s)
            for (int k = lane; k < sw; k += 64) mypos[wf[k]] = -1;
    }
    // rows with data of the node (level_table_stats sums them: one hot word for 17,000 workgroups' atomics cost 1 ms per level)
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    __syncthreads();
    int *wcnt = reinterpret_cast<int *>(pos);
    if (lane == 0) wcnt[wave] = (int)cnt;
    __syncthreads();
    if (tid == 0) node_present[n] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// Round 4: ONE workgroup per node builds every rows-sized table of the node (receptive fields of at most 32 vertices): what
// build_level_rows, build_level_inv, expand_rowscale, build_trow and build_fwd_goff built in five launches that each re-read the
// selection maps -- 1.0 of the 1.45 ms of table-building kernels per prepared 1024-molecule batch, which run beside the step of
// another handle in the loop with a new batch every step.  The source fields of the node's neighbours are staged in LDS once and the
// map of a (neighbour, position) pair is a scan of at most 32 entries by its own thread (no per-neighbour barriers); the maps stay
// in LDS for the presence masks, the transposed-row table and the gather offsets of combine-forward.
// cons_of_pair[e] = index of pair e in its source's consumer list (the inverse of cons_pair: invert_cons_pair).
// The per-consumer entries of a level's consumer lists from the list itself (round 4, second session; the host wrote them in a pass of
// its own -- phase D of gfsmp::build_batch, 2 ms of a 1024-molecule prepare -- and uploaded 24 bytes per pair): consumer c is the pair
// e = cons_pair[c] = (node n, index a); its slab of the promoted tensor, its size, its first row and a.
__global__ void build_consumer_entries(const long long *__restrict__ cons_pair, const int *__restrict__ pair_node, const int *__restrict__ node_s,
                                       const long long *__restrict__ node_pair, const long long *__restrict__ node_row,
                                       const long long *__restrict__ node_p, long long *__restrict__ cons_slab, int *__restrict__ cons_s,
                                       long long *__restrict__ cons_row, int *__restrict__ cons_a, long long pairs) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= pairs) return;
    const long long e = cons_pair[c];
    const int n = pair_node[e], sz = node_s[n], a = (int)(e - node_pair[n]);
    cons_slab[c] = node_p[n] + (long long)a * sz * sz;
    cons_s[c] = sz;
    cons_row[c] = node_row[n];
    cons_a[c] = a;
}
__global__ void invert_cons_pair(const long long *__restrict__ cons_pair, int *__restrict__ cons_of_pair, long long pairs) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < pairs) cons_of_pair[cons_pair[c]] = (int)c;
}
__global__ __launch_bounds__(128) void build_node_tables(
    const int *__restrict__ node_s, const int *__restrict__ node_mol, const long long *__restrict__ node_row,
    const long long *__restrict__ node_pair, const int *__restrict__ field, const int *__restrict__ prev_field,
    const long long *__restrict__ pair_src_pair, const int *__restrict__ pair_src_s, const int *__restrict__ mol_nv,
    const long long *__restrict__ mol_adj_off, const int *__restrict__ mol_adj, const double *__restrict__ mol_coul,
    float *__restrict__ adj, float *__restrict__ rsum, float *__restrict__ node_scale, short *__restrict__ pi,
    int *__restrict__ node_present, int swp,                                     // swp: largest field of the level below
    const int *__restrict__ cons_of_pair, const long long *__restrict__ cons_inv_off, short *__restrict__ inv,   // or null (no consumers' maps)
    float2 *__restrict__ rowscale,                                               // or null
    int *__restrict__ trow, unsigned char *__restrict__ rowflag, int *__restrict__ trowf,   // trow null: none of the three
    int2 *__restrict__ goff) {                                                   // or null
    extern __shared__ int nt_smem[];
    const int n = blockIdx.x, s = node_s[n], m = node_mol[n], V = mol_nv[m];
    const long long r0 = node_row[n], p0 = node_pair[n];
    int *f = nt_smem;                                             // [s] the node's field
    float *rs = reinterpret_cast<float *>(f + s);                 // [s] gated row sums
    float *dg = rs + s;                                           // [s] gated diagonal
    unsigned *mask = reinterpret_cast<unsigned *>(dg + s);        // [s] bit p: neighbour a's source holds the vertex of position p
    int *sf = reinterpret_cast<int *>(mask + s);                  // [s][swp] the neighbours' source fields, -1 padded
    short *spi = reinterpret_cast<short *>(sf + s * swp);         // [s][s] the maps
    const int *madj = mol_adj + mol_adj_off[m];
    const double *mc = mol_coul ? mol_coul + mol_adj_off[m] : nullptr;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < s; i += nt) f[i] = field[p0 + i];
    for (int i = tid; i < s * swp; i += nt) {
        const int a = i / swp, k = i - a * swp;
        sf[i] = k < pair_src_s[p0 + a] ? prev_field[pair_src_pair[p0 + a] + k] : -1;
    }
    __syncthreads();
    auto entry = [&](int i, int j) {
        return mc ? (float)mc[(size_t)f[i] * V + f[j]] : ((f[i] == f[j]) ? 1.f : (float)madj[(size_t)f[i] * V + f[j]]);
    };
    for (int idx = tid; idx < s * s; idx += nt) adj[r0 + idx] = entry(idx / s, idx % s);
    for (int i = tid; i < s; i += nt) {  // (entries with A <= 0 are skipped: RisiContraction_18.h:90; j in order, as the host sums)
        float acc = 0.f;
        for (int j = 0; j < s; ++j) {
            const float av = entry(i, j);
            if (av > 0.f) acc += av;
        }
        rs[i] = acc;
        rsum[p0 + i] = acc;
        const float d = entry(i, i);
        dg[i] = d > 0.f ? d : 0.f;
    }
    // the maps: pi[a][p] = position of the vertex of position p inside the field of neighbour a's source, -1 outside (:461-474)
    for (int i = tid; i < s * s; i += nt) {
        const int a = i / s, p = i - a * s, v = f[p];
        const int *row = sf + a * swp;
        int k = -1;
        for (int kk = 0; kk < swp; ++kk) k = row[kk] == v ? kk : k;   // (a field holds a vertex once)
        pi[r0 + i] = (short)k;
        spi[i] = (short)k;
        if (inv && k >= 0) inv[cons_inv_off[cons_of_pair[p0 + a]] + k] = (short)p;
    }
    __syncthreads();
    float tot = 0.f, tr = 0.f;   // (every thread forms them, in the host's order: the row factors below need them)
    for (int i = 0; i < s; ++i) {
        tot += rs[i];
        tr += dg[i];
    }
    if (tid == 0) {
        node_scale[2 * (size_t)n] = tot;
        node_scale[2 * (size_t)n + 1] = tr;
    }
    for (int a = tid; a < s; a += nt) {
        unsigned mk = 0u;
        for (int p = 0; p < s; ++p) mk |= (spi[a * s + p] >= 0 ? 1u : 0u) << p;
        mask[a] = mk;
    }
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int a = 0; a < s; ++a) cnt += __popc(mask[a]);
        node_present[n] = cnt;
    }
    for (int i = tid; i < s * s; i += nt) {
        const int x = i / s, e = i - x * s, it = e * s + x;
        if (rowscale) rowscale[r0 + i] = make_float2(tot, tr);
        const short pxe = spi[i], pex = spi[it];
        if (goff) goff[r0 + i] = make_int2(pxe >= 0 ? (int)(pair_src_pair[p0 + x] + pxe) : -1, pex >= 0 ? (int)(pair_src_pair[p0 + e] + pex) : -1);
        if (trow) {
            const long long t = r0 + it;
            trow[r0 + i] = (int)t;
            const bool own = pxe >= 0, trp = pex >= 0;
            // row (b, c) = (x, e) of the S_bc / T10 blocks has data when SOME neighbour's source holds both b and c
            unsigned both = 0u;
            for (int a = 0; a < s; ++a) both |= (mask[a] >> x) & (mask[a] >> e);
            const bool bc = (both & 1u) != 0;
            rowflag[r0 + i] = (own ? 1 : 0) | (bc ? 2 : 0);
            if (trowf)
                trowf[r0 + i] = (t < (1ll << 29)) ? (int)((unsigned)t | (own ? 0x80000000u : 0u) | (trp ? 0x40000000u : 0u) | (bc ? 0x20000000u : 0u)) : -1;
        }
    }
}

// stats = {max |tot| (float bits), max |tr|, rows with data (two words)} of a level; one workgroup, fixed order
__global__ __launch_bounds__(1024) void level_table_stats(const float *__restrict__ node_scale, const int *__restrict__ node_present,
                                                          int nodes, unsigned *__restrict__ stats) {
    __shared__ float mt[1024], mr[1024];
    __shared__ unsigned long long sc[1024];
    float a = 0.f, b = 0.f;
    unsigned long long c = 0;
    for (int n = threadIdx.x; n < nodes; n += 1024) {
        a = fmaxf(a, fabsf(node_scale[2 * (size_t)n]));
        b = fmaxf(b, fabsf(node_scale[2 * (size_t)n + 1]));
        c += (unsigned long long)node_present[n];
    }
    mt[threadIdx.x] = a, mr[threadIdx.x] = b, sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            mt[threadIdx.x] = fmaxf(mt[threadIdx.x], mt[threadIdx.x + o]);
            mr[threadIdx.x] = fmaxf(mr[threadIdx.x], mr[threadIdx.x + o]);
            sc[threadIdx.x] += sc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = __float_as_uint(mt[0]);
        stats[1] = __float_as_uint(mr[0]);
        stats[2] = (unsigned)(sc[0] & 0xffffffffull);
        stats[3] = (unsigned)(sc[0] >> 32);
    }
}

// inv[cons_inv_off[c] + k] = p  where source position k is the image of the consumer's position p (inv prefilled with -1)
__global__ __launch_bounds__(256) void build_level_inv(const long long *__restrict__ cons_pair, const int *__restrict__ pair_node,
                                                       const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                       const long long *__restrict__ node_pair, const long long *__restrict__ cons_inv_off,
                                                       const short *__restrict__ pi, short *__restrict__ inv, long long pairs) {
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= pairs) return;
    const int lane = threadIdx.x & 63;
    const long long e = cons_pair[c];
    const int n = pair_node[e], s = node_s[n], a = (int)(e - node_pair[n]);
    const short *row = pi + node_row[n] + (long long)a * s;
    short *iv = inv + cons_inv_off[c];
    for (int p = lane; p < s; p += 64) {
        const short k = row[p];
        if (k >= 0) iv[k] = (short)p;
    }
}

// trow[row of (x, e)] = row of (e, x) inside the same node (compact O layout of the fused C = 64 level, smp_level_c64.hip)
__global__ void build_trow(int *__restrict__ trow, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                           const short *__restrict__ pi, unsigned char *__restrict__ rowflag, int *__restrict__ trowf) {
    const int n = blockIdx.x, s = node_s[n];
    const long long r0 = node_row[n];
    for (int i = threadIdx.x; i < s * s; i += blockDim.x) {
        const int it = (i % s) * s + i / s;
        const long long t = r0 + it;
        trow[r0 + i] = (int)t;
        const bool own = pi[r0 + i] >= 0, tr = pi[r0 + it] >= 0;
        // row (b, c) of the S_bc / T10 blocks (sums over a of P[a,b,c]) has data when SOME source a holds both b and c: 92 % of the
        // rows at level 3 of QM9-size molecules, 71 % at level 2, 29 % at level 1 (only b == c: a level-0 field is one vertex)
        bool bc = false;
        {
            const int b = i / s, c = i % s;
            for (int a = 0; a < s && !bc; ++a) bc = pi[r0 + a * s + b] >= 0 && pi[r0 + a * s + c] >= 0;
        }
        rowflag[r0 + i] = (own ? 1 : 0) | (bc ? 2 : 0);  // bit 0: the S_ab / T6 blocks of the row are written by tables-forward
                                                          // (DevLevel::t_zeros), bit 1: its S_bc / T10 blocks are
        if (trowf)
            trowf[r0 + i] = (t < (1ll << 29)) ? (int)((unsigned)t | (own ? 0x80000000u : 0u) | (tr ? 0x40000000u : 0u) | (bc ? 0x20000000u : 0u)) : -1;
    }
}

// ---- row classes of a level (smp_rowpanel_split, CLS): the rows whose S_ab / T6 blocks hold data (bit 31 of the packed table) and the
// rows where they are structural zeros, as two lists in ascending row order, each padded to a multiple of 32 entries so that a 32-row
// panel of the product kernels holds rows of ONE class.  Buffer (ints): [0] own rows, [1] absent rows, [2..3] unused; from int 4 on the
// entries (row, the row's packed word) -- the own list, its padding, the absent list, its padding; behind room for rows + 64 entries
// the scratch words of the scan.  A padding entry repeats the last entry of its class with bit 31 of the row set: the kernel loads
// that row and stores into its scratch rows.  A stable partition in three launches: own rows per 1,024-row block, an exclusive scan of
// the block counts, the scatter.
// live_only (the driver's lists of a 64-channel level, FusedRoute::skip_empty): a third outcome -- a row with none of bits 31 / 30 / 29
// (an EMPTY row: no data in any block of T, nothing reads its gradients) goes into NEITHER list; [1] then counts the absent rows that
// are left, and a second set of block counts (behind the first) ranks them.
constexpr int kRcBlock = 1024;
__device__ __forceinline__ bool rc_kept_absent(int t, bool live_only) { return t >= 0 && (!live_only || (t & 0x60000000) != 0); }
__global__ __launch_bounds__(kRcBlock) void row_class_count(const int *__restrict__ trowf, int rows, int *__restrict__ blockcnt, int live_only) {
    const int r = blockIdx.x * kRcBlock + threadIdx.x;
    const int t = r < rows ? trowf[r] : 0;
    const int n = __syncthreads_count(r < rows && t < 0);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = n;
    if (live_only) {   // (uniform)
        const int m = __syncthreads_count(r < rows && rc_kept_absent(t, true));
        if (threadIdx.x == 0) blockcnt[gridDim.x + blockIdx.x] = m;
    }
}
__global__ __launch_bounds__(kRcBlock) void row_class_scan(int *__restrict__ blockcnt, int nb, int rows, int *__restrict__ hdr, int live_only) {
    __shared__ int part[kRcBlock];
    const int tid = threadIdx.x, per = (nb + kRcBlock - 1) / kRcBlock;
    const int i0 = tid * per < nb ? tid * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
    for (int set = 0; set < (live_only ? 2 : 1); ++set) {   // own rows; live_only: then the absent rows that are kept
        int *cnt = blockcnt + set * nb;
        int sum = 0;
        for (int i = i0; i < i1; ++i) sum += cnt[i];
        __syncthreads();
        part[tid] = sum;
        __syncthreads();
        for (int d = 1; d < kRcBlock; d <<= 1) {
            const int v = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int run = part[tid] - sum;
        for (int i = i0; i < i1; ++i) {
            const int c = cnt[i];
            cnt[i] = run;
            run += c;
        }
        if (tid == kRcBlock - 1) {
            if (set == 0) hdr[0] = part[tid], hdr[1] = rows - part[tid], hdr[2] = hdr[3] = 0;
            else hdr[1] = part[tid];
        }
    }
}
__global__ __launch_bounds__(kRcBlock) void row_class_fill(const int *__restrict__ trowf, int rows, const int *__restrict__ blockoff,
                                                           const int *__restrict__ hdr, int2 *__restrict__ ent, int live_only) {
    __shared__ int wcnt[kRcBlock / 64], wabs[kRcBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = blockIdx.x * kRcBlock + tid;
    const int t = r < rows ? trowf[r] : 0;
    const bool own = t < 0, kept = r < rows && rc_kept_absent(t, live_only != 0);
    const unsigned long long b = __ballot(own), ba = __ballot(kept);
    if (lane == 0) wcnt[w] = __popcll(b), wabs[w] = __popcll(ba);
    __syncthreads();
    int before = blockoff[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));   // own rows in front of row r
    for (int i = 0; i < w; ++i) before += wcnt[i];
    int abs_before = r - before;                                                  // absent rows in front of it: all of them, or the kept ones
    if (live_only) {   // (uniform)
        abs_before = blockoff[gridDim.x + blockIdx.x] + __popcll(ba & ((1ull << lane) - 1ull));
        for (int i = 0; i < w; ++i) abs_before += wabs[i];
    }
    if (r >= rows || (!own && !kept)) return;
    const int n_own = hdr[0], n_abs = hdr[1], own_pad = (n_own + 31) & ~31;
    const int k = own ? before : abs_before;   // the row's rank in its class
    const int at = own ? k : own_pad + k;
    ent[at] = make_int2(r, t);
    if (k == (own ? n_own : n_abs) - 1) {   // the last row of a class fills the class's padding
        const int end = own ? own_pad : own_pad + ((n_abs + 31) & ~31);
        for (int i = at + 1; i < end; ++i) ent[i] = make_int2((int)((unsigned)r | 0x80000000u), t);
    }
}

// the node of every entry of the two lists (padding entries: their row's): node_row is ascending, a bisection per entry
__global__ void row_class_nodes(const int *__restrict__ hdr, const int2 *__restrict__ ent, const long long *__restrict__ node_row, int nodes,
                                int *__restrict__ ent_node) {
    const int n_ent = ((hdr[0] + 31) & ~31) + ((hdr[1] + 31) & ~31);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ent) return;
    const long long row = ent[i].x & 0x1fffffff;
    int lo = 0, hi = nodes - 1;   // the last node whose first row is <= row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (node_row[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    ent_node[i] = lo;
}

// ---- gf_smp_prepare: the steps ------------------------------------------------------------------------------------
// The ONE way a batch's buffers are taken from the pool: the first failure is kept and every later request does nothing, so a step asks
// for its buffers in order and checks `st` at its end (and before it launches anything on them).  The ORDER of the requests is behaviour:
// upload_bytes picks the best-fitting idle block, so it decides which block backs which buffer and how far the pool grows.
struct Taker {
    gf_smp *s;
    gf_status st = GF_OK;
    template <typename T>
    void alloc(T **p, size_t count) {   // room for `count` elements, contents undefined
        if (st == GF_OK) st = upload(s, p, nullptr, count);
    }
    template <typename T, typename V>
    void put(T **p, const V &v) {   // a host table, copied on the handle's upload stream
        if (st == GF_OK) st = upload(s, p, v.empty() ? nullptr : &v[0], v.size());
    }
    template <typename T, typename V>
    void table(T **p, const V &v, size_t count) {   // a rows-sized table: the host's, or room for the one the device builds
        s->lay.device_tables ? alloc(p, count) : put(p, v);
    }
};
using Level = const gfsmp::LevelLayout;
using DevLevel = gf_smp::DevLevel;

// SMP_2D_ver6 / ver7 on the 18-slice level: the identities behind the embedding need a symmetric, non-negative adjacency (row sums =
// column sums), for `_50` the unit diagonal of a reduced adjacency (cases 25, 41, 42, 45: no Coulomb mode), and in Coulomb mode
// positive entries (RisiContraction_18 drops A <= 0 -- its `if (adj_value > 0)` -- and RisiContraction_10 does not).  A batch that
// does not qualify runs on the op-by-op `_10` / `_50` levels, which take anything the reference takes; the plan is per batch.
gf_status choose_plan(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *coulomb) {
    if (!s->dup_channels && !s->embed_auto_off) return GF_OK;
    const bool is50 = s->ucfg.nContractions == 50;
    bool embeddable = !(is50 && coulomb);
    const int *a = adj;
    const double *cm = coulomb;
    for (int m = 0; m < nMol && embeddable; ++m) {
        const int V = nVertices[m];
        if (cm)
            for (int i = 0; i < V * V && embeddable; ++i) embeddable = cm[i] > 0.0;
        for (int i = 0; i < V && embeddable; ++i)
            for (int j = i + 1; j < V; ++j)
                if (a[i * V + j] < 0 || a[i * V + j] != a[j * V + i] || (cm && cm[i * V + j] != cm[j * V + i])) {
                    embeddable = false;
                    break;
                }
        a += (size_t)V * V;
        if (cm) cm += (size_t)V * V;
    }
    return embeddable != (s->dup_channels != 0) ? smp_switch_plan(s, embeddable) : GF_OK;
}

// the batch's uploads and table-building kernels run at the LOWEST stream priority: in the loop with a new batch every step they
// share the device with the running step of another handle, which is what the loop waits for
void ensure_upload_stream(gf_smp *s) {
    if (s->upload) return;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest) {
        if (hipStreamCreateWithPriority(&s->upload, hipStreamNonBlocking, least) != hipSuccess) s->upload = nullptr;
    } else if (hipStreamCreateWithFlags(&s->upload, hipStreamNonBlocking) != hipSuccess) {
        s->upload = nullptr;
    }
    if (s->upload && hipEventCreateWithFlags(&s->ev_last, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(s->upload);
        s->upload = nullptr;
        s->ev_last = nullptr;
    }
}
hipStream_t upload_stream(const gf_smp *s) { return s->upload ? s->upload : s->ctx->stream; }

// The two ends of every prepare path.  A path refuses what it can BEFORE begin_batch (the previous batch then stays usable); between the two
// it lays the batch out on the host, assigns s->lv and takes its buffers through a Taker; a refusal there leaves the handle unprepared.
void begin_batch(gf_smp *s) {
    ensure_upload_stream(s);
    release(s);
}
// the tables are on the device when this returns (the host vectors are reused by the next batch); the context's stream is NOT waited for:
// it may be running another handle's step.  ws_need: grown by forward / backward on the compute thread (smp_internal.h)
gf_status finish_batch(gf_smp *s, size_t ws_need) {
    s->ws_need = ws_need;
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(upload_stream(s)));
    s->prepared = true;
    return GF_OK;
}
// molecule m above the configuration's max_nVertices (the paths whose buffers or parameters are sized by it), in the entry point's name
gf_status check_max_vertices(const gf_smp *s, const char *who, int m, int V) {
    if (V <= s->cfg.max_nVertices) return GF_OK;
    return fail(s->ctx, GF_ERR_INVALID, "%s: molecule %d has %d vertices, the model was created with max_nVertices = %d", who, m, V, s->cfg.max_nVertices);
}

// rows-sized level tables on the device (GF_PREP_DEVICE_TABLES=0: on the host, as rounds 1-2 built them; the parity tests hold
// the two against each other bit for bit)
void choose_table_builder(gf_smp *s, int nMol, const int *nVertices) {
    s->lay.device_tables = !env_is("GF_PREP_DEVICE_TABLES", '0');
    // build_level_rows keeps three ints per field position and four shorts per vertex of its molecule in LDS: beyond the
    // default 32 KiB window (a molecule of ~4,000 vertices) the tables are built on the host, as rounds 1-2 built all of them
    // (decided BEFORE build_batch lays the batch out for one builder or the other; round-3 advice)
    int vmax = 0;
    for (int m = 0; m < nMol; ++m) vmax = nVertices[m] > vmax ? nVertices[m] : vmax;
    const int smax = s->cfg.max_receptive_field > 0 && s->cfg.max_receptive_field < vmax ? s->cfg.max_receptive_field : vmax;
    if (sizeof(int) * (size_t)smax * 3 + sizeof(short) * 4 * (size_t)vmax + 16 > 32 * 1024) s->lay.device_tables = false;
}

// every level: node bookkeeping, the activations and their gradient; a tower reads every level out
void alloc_level_state(Taker &t, Level &h, DevLevel &d, int l) {
    const gfsmp::Config &cfg = t.s->cfg;
    const int Cl = cfg.level_channels(l);
    t.put(&d.node_s, h.node_s);
    t.put(&d.node_center, h.node_center);
    t.put(&d.mol_order, h.mol_order);
    t.put(&d.gather_items, h.gather_items);
    if (t.s->lay.device_tables) {
        t.put(&d.field, h.field);
        if (!cfg.physics) t.put(&d.node_mol, h.node_mol);   // (the towers upload it below)
    }
    if (l >= 1 && cfg.square()) t.alloc(&d.tf_recs, (size_t)h.nNodes * 2);
    t.put(&d.node_row, h.node_row);
    t.put(&d.node_pair, h.node_pair);
    t.alloc(&d.f, (size_t)h.rows * Cl);
    t.alloc(&d.df, (size_t)h.rows * Cl);
    if (!cfg.physics) return;
    t.alloc(&d.sh, (size_t)h.nNodes * Cl);   // per-node sums, their activation and gradient, the vertex -> node map
    t.alloc(&d.vf, (size_t)h.nNodes * Cl);
    t.alloc(&d.dshl, (size_t)h.nNodes * Cl);
    t.put(&d.node_of_vertex, t.s->lay.node_of_vertex[l]);
    t.put(&d.node_mol, h.node_mol);
    t.alloc(&d.keep_mask, (size_t)h.nNodes);
}

// levels >= 1, every kind: the promotion's pair tables, the consumer lists of the reverse gather, the selection maps.  The rows-sized
// ones are the host's or are built on the device (build_consumer_entries here, the node tables in build_device_tables).
gf_status alloc_level_topology(Taker &t, Level &h, DevLevel &d, int l) {
    gf_smp *s = t.s;
    const bool dev = s->lay.device_tables;
    t.put(&d.node_p, h.node_p);
    t.table(&d.adj, h.adj, (size_t)h.rows);
    t.table(&d.rsum, h.rsum, (size_t)h.pairs);
    t.table(&d.node_scale, h.rowscale, (size_t)h.nNodes * 2);
    if (dev) t.alloc(&d.node_present, (size_t)h.nNodes);
    for (size_t i = 0; !dev && i + 1 < h.rowscale.size(); i += 2) {
        d.max_tot = std::max(d.max_tot, std::fabs(h.rowscale[i]));
        d.max_tr = std::max(d.max_tr, std::fabs(h.rowscale[i + 1]));
    }
    t.alloc(&d.rowscale, (size_t)h.rows * 2);
    t.put(&d.quad_node, h.quad_node);
    t.put(&d.quad_b0, h.quad_b0);
    t.put(&d.quad_order, h.quad_order);
    t.put(&d.pair_node, h.pair_node);
    t.put(&d.pair_src_s, h.pair_src_s);
    t.table(&d.cons_s, h.cons_s, (size_t)h.pairs);
    t.table(&d.cons_a, h.cons_a, (size_t)h.pairs);
    t.put(&d.pair_src_pair, h.pair_src_pair);
    t.table(&d.cons_row, h.cons_row, (size_t)h.pairs);
    t.put(&d.cons_pair, h.cons_pair);
    if (s->cfg.nContractions != 4)   // the compact diagonal path of the 18-slice level (SMP_gamma has none of its scratch)
        for (float **p : {&d.Fdc, &d.Gc, &d.dGc, &d.dFdc}) t.alloc(p, (size_t)s->lay.level[l - 1].pairs * 2 * s->cfg.nChanels);
    t.put(&d.pair_src_row, h.pair_src_row);
    t.put(&d.cons_ptr, h.cons_ptr);
    t.table(&d.cons_slab, h.cons_slab, (size_t)h.pairs);
    if (t.st != GF_OK) return t.st;
    if (dev && h.pairs) {
        hipLaunchKernelGGL(build_consumer_entries, dim3((unsigned)((h.pairs + 255) / 256)), dim3(256), 0, upload_stream(s), d.cons_pair, d.pair_node,
                           d.node_s, d.node_pair, d.node_row, d.node_p, d.cons_slab, d.cons_s, d.cons_row, d.cons_a, (long long)h.pairs);
        GF_LAUNCH_CHECK(s->ctx, "build_consumer_entries");
    }
    t.put(&d.cons_inv_off, h.cons_inv_off);
    t.table(&d.pi, h.pi, (size_t)h.rows);
    t.table(&d.inv, h.inv, (size_t)h.inv_count);
    return t.st;
}

// fused 18-slice levels with the folded backward gather: its header and record tables (smp_fused.hip: build_gather_records)
void alloc_level_gather(Taker &t, Level &h, DevLevel &d) {
    const gfsmp::Config &cfg = t.s->cfg;
    if (!(cfg.square() && cfg.nContractions == 18 && cfg.nChanels % 4 == 0 && t.s->bwd_gather)) return;
    t.alloc(&d.cons_hdr, (size_t)h.pairs * 2);
    t.alloc(&d.cons_qrec, (size_t)h.qrec_total);
    t.put(&d.cons_qbase, h.cons_qbase);
}

// the row-panel kernel family (C = 64; 32: the split row-panel products, round 4; 16: round 5): transposed-row tables and weight images,
// and for an 18-slice level the row panels of the fused forward (smp_level_c64_fwd.hip) with their partial sums and maxima
void alloc_level_panels(Taker &t, Level &h, DevLevel &d, int l) {
    const gfsmp::Config &cfg = t.s->cfg;
    const int L = cfg.nLevels, C = cfg.nChanels;
    // (C = 128, the plain 18-slice model: the tables and four sets of weight images for the sub-block passes of the product kernels)
    const bool c128 = C == 128 && cfg.nContractions == 18 && !cfg.physics && smp_c128_switch();
    if (!(cfg.square() && (smp_panel_channels(C) || c128) && h.rows < 0x7fffffffll)) return;
    t.alloc(&d.trow, (size_t)h.rows);
    t.alloc(&d.trowf, (size_t)h.rows);
    // (row classes of the masked products; the driver's lists leave the empty rows out: smp_build_row_classes, live_only)
    if (C == 64 && cfg.nContractions == 18 && h.rows < (1ll << 29)) t.alloc(&d.rowcls, smp_row_class_ints((int)h.rows, true));
    // (the top level of a plain model: its backward products form dz from the read-out's per-node vector -- the node of every list entry)
    if (d.rowcls && l == L && !cfg.physics) t.alloc(&d.rowcls_node, (size_t)h.rows + 64);
    unsigned char *img = nullptr;
    t.alloc(&img, smp_split_image_bytes(C));
    d.wimg = img;
    t.alloc(&d.rowflag, (size_t)h.rows);
    if (c128) return;   // (the panel kernels of tables / combine are not built for 128 channels)
    if (!(cfg.nContractions == 18 && h.rows * 256 < 0x3fffffffll && !h.buckets.empty() && h.buckets.back().s <= kFusedMaxField)) return;
    // a node of size s has ceil(s / max(1, 32 / s)) panels
    const int np = h.npanels;   // (page-locked table of the layout: no wait for the copy)
    const size_t np1 = (size_t)(np > 0 ? np : 1);   // (a level whose nodes are ALL above 32 positions has no panel: the tables exist all the same)
    d.fwd_npanels = np;
    t.put(&d.node_panel, h.node_panel);
    t.alloc(&d.fwd_pan, np1);
    if (l == L || cfg.physics) t.alloc(&d.psum, np1 * C);   // (the top level -- every level of a tower: the readout's partial sums)
    if (l < L) t.alloc(&d.pmax, np1 * C);   // (below the top level: the per-panel channel maxima the level above scales its weight-gradient operands with)
    t.alloc(&d.dzmax, (h.quad_node.size() + np1) * 64);   // (panels, then the workgroups of the nodes above 32 positions)
    t.alloc(&d.fwd_pan_node, np1);
    t.alloc(&d.fwd_goff, (size_t)h.rows);
    if (C == 64) t.alloc(&d.sgn, (size_t)h.rows * 2);   // (the sign words of z_l: 8 bytes per row)
    if (C == 64 && d.rowcls) t.alloc(&d.pan_live, np1);   // (the panels' live-row words: FusedRoute::skip_empty)
}

// the contraction's output and what the level's kind works in beside it
void alloc_level_scratch(Taker &t, Level &h, DevLevel &d, int l) {
    const gfsmp::Config &cfg = t.s->cfg;
    const size_t C = cfg.nChanels, Cl = cfg.level_channels(l), Cp = cfg.level_channels(l - 1), pairs = h.pairs, nodes = h.nNodes;
    if (cfg.nContractions == 4) {
        // a `_4` level: T [rows][4 Cp] op by op, G / dG [rows of level l - 1][4 Cc] on the gamma level (Cc <= Cp); then the gamma level's
        // weight views [8 Cp Cc] and its weight-gradient image [4 Cp Cc] (Cp = Cc = C unless a tower)
        t.alloc(&d.Q, (size_t)std::max<int64_t>(h.rows, t.s->lay.level[l - 1].rows) * 4 * Cp);
        t.alloc(&d.Wst, 8 * Cp * Cl);
        t.alloc(&d.dWst, 4 * Cp * Cl);
        return;
    }
    t.alloc(&d.Q, (size_t)h.rows * std::max(18, cfg.nContractions) * Cp);
    if (!cfg.square()) return;
    // fused level (smp_fused.hip): small per-(node, x) / per-node tables and the stacked weights
    const struct { float **p; size_t n; } bufs[] = {
        {&d.Vt, pairs * 4 * C}, {&d.dVt, pairs * 4 * C}, {&d.St, nodes * 4 * C}, {&d.dSt, nodes * 4 * C}, {&d.scal, pairs * 4 * C},
        {&d.Vout, pairs * C}, {&d.dVout, pairs * C}, {&d.Sout, nodes * C}, {&d.dSout, nodes * C}, {&d.dSpart, pairs * C},
        {&d.dbpart, pairs * C}, {&d.Wst, 18 * C * C}, {&d.dWst, 18 * C * C}};
    for (const auto &b : bufs) t.alloc(b.p, b.n);
}

// all the device buffers of level l; *maxp, *contract_ws: the promoted stack and the contraction workspace the level would need
gf_status alloc_level(gf_smp *s, int l, long long *maxp, size_t *contract_ws) {
    Taker t = {s};
    Level &h = s->lay.level[l];
    DevLevel &d = s->lv[l];
    alloc_level_state(t, h, d, l);
    if (l == 0) return t.st;
    const gf_status st = alloc_level_topology(t, h, d, l);   // (its own status: a failed launch check is not in t.st)
    if (st != GF_OK) return st;
    alloc_level_gather(t, h, d);
    alloc_level_panels(t, h, d, l);
    alloc_level_scratch(t, h, d, l);
    const int Cp = s->cfg.level_channels(l - 1);
    *maxp = std::max<long long>(*maxp, h.ppos * Cp);
    for (const gfsmp::Bucket &bk : h.buckets) *contract_ws = std::max(*contract_ws, gf_contract_workspace_bytes(s->cfg.nContractions, bk.s, Cp, bk.count));
    *contract_ws = std::max(*contract_ws, r18_ragged_workspace_bytes((long long)h.rows, (long long)h.pairs, Cp));
    return t.st;
}

// device-built tables: the molecules' adjacency matrices go up, then the rows-sized tables of every level (kernels above)
gf_status build_device_tables(gf_smp *s, bool coulomb) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::BatchLayout &B = s->lay;
    const int L = s->cfg.nLevels, vmax = B.max_vertices;
    hipStream_t up = upload_stream(s);
    Taker t = {s};
    t.put(&s->mol_nv, B.mol_nv);
    t.put(&s->mol_adj, B.mol_adj);
    t.put(&s->mol_adj_off, B.mol_adj_off);
    if (coulomb) t.put(&s->mol_coul, B.mol_coul);
    t.alloc(&s->tab_stats, (size_t)4 * (L + 1));  // per level: max |tot|, max |tr| (float bits), rows with data (64 bit)
    if (t.st != GF_OK) return t.st;
    GF_HIP_TRY(ctx, hipMemsetAsync(s->tab_stats, 0, sizeof(unsigned) * 4 * (L + 1), up));
    for (int l = 1; l <= L; ++l) {
        const gfsmp::LevelLayout &h = B.level[l];
        gf_smp::DevLevel &d = s->lv[l];
        const int smax = h.buckets.empty() ? 1 : h.buckets.back().s;
        const size_t lds = sizeof(int) * (size_t)smax * 3 + sizeof(short) * 4 * (size_t)vmax + 16;
        if (lds > 32 * 1024)   // (cannot happen: choose_table_builder chose the host builder for such a batch)
            return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare: a receptive field of %d vertices in a molecule of %d", smax, vmax);
        // (the split-operand weight gradients read the level's largest |tot|, |tr| from its statistics words: no read-back, the preparing
        //  thread does not wait for its uploads)
        unsigned *stats = s->tab_stats + 4 * l;
        d.row_max = stats;
        if (h.inv_count) GF_HIP_TRY(ctx, hipMemsetAsync(d.inv, 0xff, sizeof(short) * (size_t)h.inv_count, up));
        // one kernel for all the node's tables where the fields fit its LDS image and its 32-bit presence masks (build_node_tables)
        const int swp = B.level[l - 1].buckets.empty() ? 1 : B.level[l - 1].buckets.back().s;
        const size_t lds_nt = sizeof(int) * (size_t)smax * (4 + (size_t)swp) + sizeof(short) * (size_t)smax * smax + 16;
        d.node_tables_merged = smax <= 32 && lds_nt <= 32 * 1024 && h.pairs > 0 && h.pairs < 0x7fffffffll;
        if (d.node_tables_merged) {
            t.alloc(&d.cons_of_pair, (size_t)h.pairs);
            if (t.st != GF_OK) return t.st;
            hipLaunchKernelGGL(invert_cons_pair, dim3((unsigned)((h.pairs + 255) / 256)), dim3(256), 0, up, d.cons_pair, d.cons_of_pair,
                               (long long)h.pairs);
            GF_LAUNCH_CHECK(ctx, "invert_cons_pair");
            hipLaunchKernelGGL(build_node_tables, dim3(h.nNodes), dim3(128), lds_nt, up, d.node_s, d.node_mol, d.node_row, d.node_pair,
                               d.field, s->lv[l - 1].field, d.pair_src_pair, d.pair_src_s, s->mol_nv, s->mol_adj_off, s->mol_adj, s->mol_coul,
                               d.adj, d.rsum, d.node_scale, d.pi, d.node_present, swp, d.cons_of_pair, d.cons_inv_off, d.inv,
                               reinterpret_cast<float2 *>(d.rowscale), d.trow, d.rowflag, d.trowf, d.fwd_goff);
            GF_LAUNCH_CHECK(ctx, "build_node_tables");
        } else {
            hipLaunchKernelGGL(build_level_rows, dim3(h.nNodes), dim3(256), lds, up, d.node_s, d.node_mol, d.node_row, d.node_pair, d.field,
                               s->lv[l - 1].field, d.pair_src_pair, d.pair_src_s, s->mol_nv, s->mol_adj_off, s->mol_adj, s->mol_coul, d.adj,
                               d.rsum, d.node_scale, d.pi, d.node_present, vmax);
            GF_LAUNCH_CHECK(ctx, "build_level_rows");
            if (h.pairs) {
                hipLaunchKernelGGL(build_level_inv, dim3((unsigned)((h.pairs + 3) / 4)), dim3(256), 0, up, d.cons_pair, d.pair_node, d.node_s,
                                   d.node_row, d.node_pair, d.cons_inv_off, d.pi, d.inv, (long long)h.pairs);
                GF_LAUNCH_CHECK(ctx, "build_level_inv");
            }
        }
        hipLaunchKernelGGL(level_table_stats, dim3(1), dim3(1024), 0, up, d.node_scale, d.node_present, h.nNodes, stats);
        GF_LAUNCH_CHECK(ctx, "level_table_stats");
    }
    return GF_OK;
}

// (the node tables went up on the handle's upload stream: the row factors, the fused levels' records and the transposed-row tables are built
//  there too, behind them)
gf_status build_row_tables(gf_smp *s) {
    hipStream_t up = upload_stream(s);
    for (int l = 1; l <= s->cfg.nLevels; ++l) {
        const gf_smp::DevLevel &d = s->lv[l];
        const int nNodes = s->lay.level[l].nNodes;
        const bool merged = d.node_tables_merged;   // (row factors, transposed-row tables and gather offsets are in place)
        if (!merged)
            hipLaunchKernelGGL(expand_rowscale, dim3(nNodes), dim3(64), 0, up, reinterpret_cast<float2 *>(d.rowscale),
                               reinterpret_cast<const float2 *>(d.node_scale), d.node_s, d.node_row);
        gf_status st = smp_build_gather_records(s, l, up);
        if (st == GF_OK) st = smp_build_tf_records(s, l, up);
        if (st == GF_OK) st = smp_fwd_fused_build_tables(s, l, up, !merged);
        if (st != GF_OK) return st;
        if (d.trow && !merged) hipLaunchKernelGGL(build_trow, dim3(nNodes), dim3(64), 0, up, d.trow, d.node_s, d.node_row, d.pi, d.rowflag, d.trowf);
        if (d.rowcls) st = smp_build_row_classes(s->ctx, up, d.trowf, (int)s->lay.level[l].rows, d.rowcls, true);
        if (st == GF_OK && d.pan_live) st = smp_build_pan_live(s, l, up);
        if (st == GF_OK && d.rowcls_node) st = smp_build_row_class_nodes(s->ctx, up, d.rowcls, (int)s->lay.level[l].rows, d.node_row, nNodes, d.rowcls_node);
        if (st != GF_OK) return st;
    }
    return GF_OK;
}

// the level-0 input, the read-out and the per-molecule buffers
gf_status alloc_readout(gf_smp *s, int nMol) {
    const gfsmp::BatchLayout &B = s->lay;
    const int L = s->cfg.nLevels, C = s->cfg.top_channels();   // (the read-out's width: nChanels but for SMP_1D_ver2 / ver3)
    const gfsmp::LevelLayout &top = B.level[L];
    Taker t = {s};
    t.put(&s->x, B.x);
    // scratch words of the fused levels' weight gradients (channel maxima, exact column bounds; a 64-channel level keeps only its maxima);
    // 128 channels: the plain 18-slice model's four sub-block launches
    if (!s->cfg.per_size() && s->cfg.square() && (smp_panel_channels(C) || (C == 128 && s->cfg.nContractions == 18 && smp_c128_switch())))
        t.alloc(&s->wbound, smp_wgrad_words(C, C != 64) * (size_t)(L + 1));
    t.alloc(&s->sh, (size_t)top.nNodes * C);
    t.alloc(&s->vf, (size_t)top.nNodes * C);
    t.alloc(&s->dsh, (size_t)top.nNodes * C);
    t.alloc(&s->g, (size_t)nMol * (s->cfg.physics ? feature_width(s->cfg) : (size_t)C));
    t.alloc(&s->yhat, (size_t)nMol);
    t.alloc(&s->dy, (size_t)nMol);
    if (s->cfg.nClass) {   // classifier read-out (smp_readout_classes.hip)
        t.alloc(&s->cls_scores, (size_t)nMol * s->cfg.nClass);
        t.alloc(&s->cls_prob, (size_t)nMol * s->cfg.nClass);
        t.alloc(&s->cls_dz, (size_t)nMol * s->cfg.nClass);
        t.alloc(&s->cls_dg, (size_t)nMol * C);
    }
    t.put(&s->top_node_mol, top.node_mol);
    t.put(&s->mol_ptr, B.mol_first_vertex);      // [nMol + 1]: the vertices of a molecule are contiguous
    t.put(&s->mol_nodes, B.top_node_of_vertex);  // [vertices = nodes of level L]
    long long maxrows = 0, maxpairs = 0;
    for (int l = 0; l <= L; ++l) {
        maxrows = std::max(maxrows, (long long)B.level[l].rows);
        maxpairs = std::max(maxpairs, (long long)B.level[l].pairs);
    }
    s->colpart_rows = (size_t)((maxrows + 1023) / 1024 + (maxpairs + 255) / 256 + 2);
    s->colpart_rows = std::max(s->colpart_rows, (size_t)256 * (L + 1));  // fused levels: up to 256 column partials per level
    t.alloc(&s->colpart, s->colpart_rows * C);
    return t.st;
}

// ---- the field levels (SMP_theta, SMP_1D*, SMP_2D / ver4 / ver5, Unrestricted_*): the host builds the batch and the level's own (node, child)
// tables (gfsmp::build_batch_theta); the device gets those, the activations and the family's buffers -- none of the 18-slice or gamma ones ----
// every level: node bookkeeping, the activations and their gradient; a tower reads every level out
void alloc_field_state(Taker &t, Level &h, DevLevel &d, int l) {
    const size_t Cl = t.s->cfg.level_channels(l), nodes = h.nNodes;
    t.put(&d.node_s, h.node_s);
    t.put(&d.node_row, h.node_row);
    t.put(&d.node_mol, h.node_mol);
    t.alloc(&d.f, (size_t)h.rows * Cl);
    t.alloc(&d.df, (size_t)h.rows * Cl);
    if (!t.s->cfg.physics) return;
    t.alloc(&d.sh, nodes * Cl);   // per-node sums, their activation and gradient, the vertex -> node map
    t.alloc(&d.vf, nodes * Cl);
    t.alloc(&d.dshl, nodes * Cl);
    t.put(&d.node_of_vertex, t.s->lay.node_of_vertex[l]);
}
// levels >= 1, every family: the (node, child) tables of smp_prep.h
void alloc_field_tables(Taker &t, Level &h, DevLevel &d) {
    t.put(&d.th_child_ptr, h.th_child_ptr);
    t.put(&d.th_src_row, h.th_src_row);
    t.put(&d.th_src_s, h.th_src_s);
    t.put(&d.th_pi_off, h.th_pi_off);
    t.put(&d.th_pi, h.th_pi);
    t.put(&d.th_cons_ptr, h.th_cons_ptr);
    t.put(&d.th_cons_row, h.th_cons_row);
    t.put(&d.th_cons_s, h.th_cons_s);
    t.put(&d.th_cons_node, h.th_cons_node);
    t.put(&d.th_inv_off, h.th_inv_off);
    t.put(&d.th_inv, h.th_inv);
    t.put(&d.th_bucket, h.th_bucket);
    t.put(&d.th_weight, h.th_weight);
}
// SMP_theta (smp_level_theta.hip): the reverse sweep's per-node sums, A, B, G / dG and the weight views
void alloc_theta_level(Taker &t, Level &h, DevLevel &d, int l) {
    const size_t Cl = t.s->cfg.level_channels(l), Cp = t.s->cfg.level_channels(l - 1), nodes = h.nNodes;
    t.alloc(&d.th_node, nodes * 3 * Cl);
    t.alloc(&d.th_A, (size_t)h.rows * Cl);
    t.alloc(&d.th_B, nodes * Cl);
    t.alloc(&d.Q, (size_t)t.s->lay.level[l - 1].rows * 2 * Cl);   // G, then dG: [rows of level l - 1][2 Cc]
    t.alloc(&d.Wst, 4 * Cp * Cl);                                 // the weight views [Cp][2 Cc] and [2 Cc][Cp]
    t.alloc(&d.dWst, 2 * Cp * Cl);
}
// SMP_1D* (smp_level_1d.hip): A = S and B = sumS are Cp wide; a matrix, and so G / dG and the weight views, only in ver3
void alloc_1d_level(Taker &t, Level &h, DevLevel &d, int l) {
    const size_t Cl = t.s->cfg.level_channels(l), Cp = t.s->cfg.level_channels(l - 1), nodes = h.nNodes;
    t.alloc(&d.th_node, nodes * 3 * Cl);
    t.alloc(&d.th_A, (size_t)h.rows * Cp);
    t.alloc(&d.th_B, nodes * Cp);
    if (t.s->cfg.first_order != 4) return;
    t.alloc(&d.Q, (size_t)t.s->lay.level[l - 1].rows * 2 * Cp);   // [rows of level l - 1][2 Cp]
    t.alloc(&d.Wst, 4 * Cp * Cp);                                 // [K_eye | K_one] as [Cp][2 Cp], and its transpose
    t.alloc(&d.dWst, 2 * Cp * Cp);
}
// SMP_2D / ver4 (smp_level_2d.hip): S [rows][Cp], col and the reverse sweep's column partials per (node, column); SMP_2D_ver5
// (smp_level_2d_ver5.hip) beside them: the tables of its projections, u, dO, dE and the partials of dK_l
void alloc_steerable_level(Taker &t, Level &h, DevLevel &d, int l) {
    const size_t Cl = t.s->cfg.level_channels(l), Cp = t.s->cfg.level_channels(l - 1);
    const size_t cols = h.nNodes ? (size_t)(h.node_pair.back() + h.node_s.back()) : 0;   // sum s
    t.put(&d.node_pair, h.node_pair);
    t.put(&d.adj, h.adj);
    t.alloc(&d.th_A, (size_t)h.rows * Cp);
    t.alloc(&d.th_B, cols * Cp);
    t.alloc(&d.th_node, cols * (Cl + 3 * Cp));
    t.alloc(&d.part2d, h.buckets.size() * 16 * (Cl + 3 * Cp));   // [buckets][kSplit2d row chunks][Cc + 3 Cp]
    if (t.s->cfg.steerable_2d != 5) return;
    t.alloc(&d.v5_row_cs, (size_t)h.rows);
    t.alloc(&d.v5_col_s, cols);
    t.alloc(&d.v5_u, cols * Cp);
    t.alloc(&d.v5_dO, cols * Cp);
    t.alloc(&d.Q, (size_t)h.rows * Cp);
    t.alloc(&d.v5_dKpart, smp_2d_ver5_wgrad_chunks((long long)h.rows, (long long)cols) * Cp * Cp);
}
// Unrestricted_* (smp_level_unrestricted.hip): S and dS [rows][Cp], the chunk partials of the per-size entries; form 3: adj, columns
void alloc_unrestricted_level(Taker &t, Level &h, DevLevel &d, int l) {
    const size_t Cp = t.s->cfg.level_channels(l - 1);
    t.alloc(&d.th_A, (size_t)h.rows * Cp);
    t.alloc(&d.Q, (size_t)h.rows * Cp);
    t.put(&d.un_part_off, h.un_part_off);
    t.alloc(&d.part2d, (size_t)h.un_part_off.back());
    if (t.s->cfg.unrestricted != 3) return;
    t.put(&d.node_pair, h.node_pair);
    t.put(&d.adj, h.adj);
    t.alloc(&d.th_node, (h.nNodes ? (size_t)(h.node_pair.back() + h.node_s.back()) : 0) * 2 * Cp);
}

gf_status smp_theta_prepare(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature) {
    const gfsmp::Config &cfg = s->cfg;
    gf_status st = GF_OK;
    for (int m = 0; m < nMol && st == GF_OK; ++m) st = check_max_vertices(s, "gf_smp_prepare", m, nVertices[m]);
    if (st != GF_OK) return st;
    begin_batch(s);
    gfsmp::build_batch_theta(cfg, nMol, nVertices, adj, feature, &s->lay);
    const int L = cfg.nLevels;
    for (int l = 0; l <= L; ++l)
        if (s->lay.level[l].rows > 0x7fffffffll || (!s->lay.level[l].buckets.empty() && s->lay.level[l].buckets.back().s > 32767))
            return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare: level %d is beyond the level's int16 positions / 2^31 rows", l);
    s->lv.assign(L + 1, DevLevel());
    const auto family = cfg.unrestricted ? alloc_unrestricted_level : cfg.steerable_2d ? alloc_steerable_level
                        : cfg.first_order >= 2 ? alloc_1d_level : alloc_theta_level;
    Taker t = {s};
    for (int l = 0; l <= L; ++l) {
        alloc_field_state(t, s->lay.level[l], s->lv[l], l);
        if (l == 0) continue;
        alloc_field_tables(t, s->lay.level[l], s->lv[l]);
        family(t, s->lay.level[l], s->lv[l], l);
    }
    if (t.st != GF_OK) return t.st;
    st = alloc_readout(s, nMol);
    return st != GF_OK ? st : finish_batch(s, 1 << 20);   // (the GEMMs grow the context's workspace for their split-K partials themselves)
}

// ---- the neighbourhood levels (NeuralFingerprint, GCN_*, GRU_GCN_*; smp_level_neighbourhood.hip): the host builds hop distances, the
// shell-sum features and one neighbour list (with its transpose) per distinct radius (gfsmp::build_batch_neighbourhood); the device gets those
// and one [vertices][H] buffer per level and quantity -- none of the field, selection or reduced-adjacency tables.  A distance handle
// (cfg.distance_channel; `distance` = the molecules' V x V matrices of doubles back to back) gets the same buffers a second time for its
// distance channel (gf_smp::lvd, the lists shared) and that channel's input rows, sorted on the device (smp_level_distance.hip) ----
struct DevList {
    long long *ptr = nullptr, *tptr = nullptr;
    int *idx = nullptr, *tidx = nullptr;
};
struct NbhHostTables {   // the host tables this path builds itself: alive until the upload stream has been waited for
    std::vector<long long> dist_off, gram_off, id_ptr;
    std::vector<float> gram_adj;
    std::vector<int> id_idx;
};
// what is refused before the previous batch is let go, molecule by molecule; *dist_count: the entries of `distance`
gf_status check_neighbourhood_batch(const gf_smp *s, const char *who, int nMol, const int *nVertices, const double *distance, size_t *dist_count) {
    for (int m = 0; m < nMol; ++m) {
        const gf_status st = check_max_vertices(s, who, m, nVertices[m]);
        if (st != GF_OK) return st;
        if (!distance) continue;   // (every entry finite, before anything is launched)
        const size_t n = (size_t)nVertices[m] * (size_t)nVertices[m];
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(distance[*dist_count + i]))
                return fail(s->ctx, GF_ERR_INVALID, "gf_smp_prepare_distance: molecule %d has a distance entry that is not finite (row %zu, column %zu)",
                            m, i / (size_t)nVertices[m], i % (size_t)nVertices[m]);
        *dist_count += n;
    }
    return GF_OK;
}
void put_neighbour_lists(Taker &t, std::vector<DevList> &lists) {
    const gfsmp::BatchLayout &B = t.s->lay;
    lists.resize(B.nb_lists.size());
    for (size_t k = 0; k < lists.size(); ++k) {
        t.put(&lists[k].ptr, B.nb_lists[k].ptr);
        t.put(&lists[k].idx, B.nb_lists[k].idx);
        t.put(&lists[k].tptr, B.nb_lists[k].tptr);
        t.put(&lists[k].tidx, B.nb_lists[k].tidx);
    }
}
// level l of one channel (gf_smp::lv, and lvd of a distance handle) on the lists of the level's radius
void alloc_neighbourhood_level(Taker &t, DevLevel &d, int l, const std::vector<DevList> &lists, size_t nV) {
    const gfsmp::Config &cfg = t.s->cfg;
    const size_t H = (size_t)cfg.nChanels;
    const bool pairs = cfg.neighbourhood == 3 || cfg.neighbourhood == 5;   // RisiLayer2D: A, T, Tt and the three quantities of its closed-form reverse
    t.alloc(&d.f, nV * H);
    t.alloc(&d.df, nV * H);
    if (pairs) t.alloc(&d.nb_T, nV);
    if (l == 0) return;
    const size_t k = (size_t)t.s->lay.nb_list_of_level[l];
    d.nb_ptr = lists[k].ptr, d.nb_idx = lists[k].idx, d.nb_tptr = lists[k].tptr, d.nb_tidx = lists[k].tidx;
    t.alloc(&d.th_A, nV * H);
    t.alloc(&d.Q, nV * H);
    if (cfg.gated())   // the GRU cell's gates and what its weight gradients read (smp_level_gru.hip)
        for (float **p : {&d.gru_z, &d.gru_r, &d.gru_c, &d.gru_q, &d.gru_dz, &d.gru_dr, &d.gru_dc, &d.gru_direct}) t.alloc(p, nV * H);
    if (cfg.third_order()) {   // the selection record, the longest list, and form 6's pooled vector (smp_level_third.hip)
        const auto &lp = t.s->lay.nb_lists[k].ptr;
        long long longest = 0;
        for (size_t v = 0; v + 1 < lp.size(); ++v) longest = lp[v + 1] - lp[v] > longest ? lp[v + 1] - lp[v] : longest;
        d.nb_max_members = (int)longest;
        t.alloc(&d.nb_sel, nV * H);
        if (!cfg.gated()) t.alloc(&d.nb_pool, nV * H);
    }
    if (pairs) {
        t.alloc(&d.th_B, nV * H);
        t.alloc(&d.th_node, nV * H);
        t.alloc(&d.nb_Tt, nV);
        t.alloc(&d.nb_sA, nV);
    }
}
// a distance handle: the molecules' distance matrices, their offsets and room for the sorted input rows x_d (smp_level_distance.hip)
void put_distance_inputs(Taker &t, int nMol, const int *nVertices, const double *distance, size_t dist_count, size_t nV, NbhHostTables &host) {
    gf_smp *s = t.s;
    host.dist_off.resize((size_t)nMol);
    long long o = 0;
    for (int m = 0; m < nMol; ++m) {
        host.dist_off[(size_t)m] = o;
        o += (long long)nVertices[m] * nVertices[m];
    }
    if (t.st == GF_OK) t.st = upload(s, &s->mol_dist, distance, dist_count);
    t.put(&s->mol_dist_off, host.dist_off);
    t.alloc(&s->xd, nV * (size_t)s->cfg.max_nVertices);
}
// GCA_1D: the adjacency VALUES as floats, the molecules' offsets, room for the Gram matrices (smp_level_readouts.hip)
void put_gram_inputs(Taker &t, int nMol, const int *nVertices, const int *adj, NbhHostTables &host) {
    gf_smp *s = t.s;
    host.gram_off.assign((size_t)nMol + 1, 0);
    for (int m = 0; m < nMol; ++m) host.gram_off[(size_t)m + 1] = host.gram_off[(size_t)m] + (long long)nVertices[m] * nVertices[m];
    host.gram_adj.resize((size_t)host.gram_off[(size_t)nMol]);
    for (size_t i = 0; i < host.gram_adj.size(); ++i) host.gram_adj[i] = (float)adj[i];
    t.put(&s->gram_adj, host.gram_adj);
    t.put(&s->gram_off, host.gram_off);
    t.alloc(&s->gram, host.gram_adj.size());
    s->gram_count = host.gram_adj.size();
}
// form 6: the list N(v) = {v}
void put_identity_list(Taker &t, size_t nV, NbhHostTables &host) {
    host.id_ptr.resize(nV + 1);
    host.id_idx.resize(nV);
    for (size_t v = 0; v <= nV; ++v) host.id_ptr[v] = (long long)v;
    for (size_t v = 0; v < nV; ++v) host.id_idx[v] = (int)v;
    t.put(&t.s->nb_id_ptr, host.id_ptr);
    t.put(&t.s->nb_id_idx, host.id_idx);
}

gf_status neighbourhood_prepare(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature, const double *distance) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &cfg = s->cfg;
    size_t dist_count = 0;
    gf_status st = check_neighbourhood_batch(s, distance ? "gf_smp_prepare_distance" : "gf_smp_prepare", nMol, nVertices, distance, &dist_count);
    if (st != GF_OK) return st;
    begin_batch(s);
    gfsmp::build_batch_neighbourhood(cfg, nMol, nVertices, adj, feature, &s->lay);
    const gfsmp::BatchLayout &B = s->lay;
    const int L = cfg.nLevels;
    const size_t nV = (size_t)B.mol_first_vertex[nMol], H = (size_t)cfg.nChanels;
    for (const gfsmp::BatchLayout::NeighbourList &nl : B.nb_lists)
        if (nl.idx.size() > 0x7fffffffull) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare: a neighbour list beyond 2^31 entries");
    s->lv.assign(L + 1, DevLevel());
    s->lvd.assign(distance ? L + 1 : 0, DevLevel());
    Taker t = {s};
    std::vector<DevList> lists;
    NbhHostTables host;
    put_neighbour_lists(t, lists);
    for (std::vector<DevLevel> *channel : {&s->lv, &s->lvd})   // (then the distance channel's levels)
        for (size_t l = 0; l < channel->size(); ++l) alloc_neighbourhood_level(t, (*channel)[l], (int)l, lists, nV);
    t.put(&s->x, B.x);
    t.alloc(&s->g, (size_t)nMol * (size_t)cfg.top_channels());
    t.alloc(&s->yhat, (size_t)nMol);
    t.alloc(&s->dy, (size_t)nMol);
    if (distance) put_distance_inputs(t, nMol, nVertices, distance, dist_count, nV, host);
    if (cfg.readout == 2) put_gram_inputs(t, nMol, nVertices, adj, host);
    if (cfg.gated())   // the gated read-out's two factors per vertex and their gradients
        for (float **p : {&s->gru_s, &s->gru_t, &s->gru_ds, &s->gru_dt}) t.alloc(p, nV * H);
    t.put(&s->top_node_mol, B.nb_vertex_mol);
    t.put(&s->mol_ptr, B.mol_first_vertex);
    if (cfg.neighbourhood == 6) put_identity_list(t, nV, host);
    if (t.st != GF_OK) return t.st;
    if (distance)   // x_d: every vertex's column, padded and sorted, behind the uploads on the handle's stream
        st = smp_distance_rows_launch(ctx, upload_stream(s), (int)nV, cfg.max_nVertices, s->mol_dist, s->mol_dist_off, s->mol_ptr, s->top_node_mol, s->xd);
    // (the TN products of dW1_l / dW2_l grow the context's workspace for their split-K partials themselves)
    return st != GF_OK ? st : finish_batch(s, 1 << 20);
}

// ---- the matrix-form handles (LCNN, GCN_MW; smp_level_rowlist.hip): the host builds x and the level's row lists, forward and transposed
// (gfsmp::build_batch_matrix_form); the device gets those and one activation / gradient buffer per level ----
void put_row_lists(Taker &t, bool lcnn) {
    gf_smp *s = t.s;
    const auto &rl = s->lay.rl;
    t.put(&s->rl_fwd.ptr, rl.ptr);
    t.put(&s->rl_fwd.src, rl.src);
    t.put(&s->rl_fwd.slot, rl.slot);
    t.put(&s->rl_fwd.coef, rl.coef);
    t.put(&s->rl_bwd.ptr, rl.tptr);
    t.put(&s->rl_bwd.src, rl.tsrc);
    t.put(&s->rl_bwd.slot, rl.tslot);
    t.put(&s->rl_bwd.coef, rl.tcoef);
    if (lcnn) {
        t.put(&s->rl_fwd.sptr, rl.sptr);
        t.put(&s->rl_bwd.sptr, rl.tsptr);
    } else {   // one slot: a row's entries are the slot's
        s->rl_fwd.sptr = s->rl_fwd.ptr;
        s->rl_bwd.sptr = s->rl_bwd.ptr;
    }
}
// the two convolutions' activations and gradients, the dense layer and its gradient; returns the weight gradients' partial images in bytes
size_t alloc_lcnn(Taker &t, size_t R, int nMol) {
    gf_smp *s = t.s;
    const gfsmp::Config &cfg = s->cfg;
    const size_t H = (size_t)cfg.nChanels, C2 = (size_t)cfg.nChanels2, k = (size_t)cfg.nNeighbors;
    t.alloc(&s->lv[1].f, R * H);
    t.alloc(&s->lv[1].df, R * H);
    t.alloc(&s->lv[2].f, R * C2);
    t.alloc(&s->lv[2].df, R * C2);
    t.alloc(&s->lv[2].Q, (size_t)nMol * cfg.nDense);
    t.alloc(&s->g, (size_t)nMol * cfg.nDense);
    return std::max(smp_rowlist_wgrad_ws_bytes((int)R, (int)(k * cfg.fdim()), (int)H), smp_rowlist_wgrad_ws_bytes((int)R, (int)(k * H), (int)C2));
}
size_t alloc_gcn_mw(Taker &t, size_t R, int nMol) {
    gf_smp *s = t.s;
    const size_t H = (size_t)s->cfg.nChanels;
    for (int l = 0; l <= s->cfg.nLevels; ++l) {
        t.alloc(&s->lv[l].f, R * H);
        t.alloc(&s->lv[l].df, R * H);
    }
    t.alloc(&s->g, (size_t)nMol * H);
    return std::max(smp_rowlist_wgrad_ws_bytes((int)R, s->cfg.fdim(), (int)H), smp_rowlist_wgrad_ws_bytes((int)R, (int)H, (int)H));
}

gf_status smp_matrix_form_prepare(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &cfg = s->cfg;
    const bool lcnn = cfg.matrix_form == 1;
    long long rows = 0, entries = 0;
    for (int m = 0; m < nMol; ++m) {
        const gf_status st = check_max_vertices(s, "gf_smp_prepare", m, nVertices[m]);
        if (st != GF_OK) return st;
        rows += lcnn ? cfg.max_nVertices : nVertices[m];
        entries += lcnn ? (long long)cfg.max_nVertices * cfg.nNeighbors : (long long)nVertices[m] * nVertices[m];   // (an upper bound)
    }
    if (rows > 0x7fffffffll || entries > 0x7fffffffll)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare: a matrix-form batch of %lld rows and up to %lld list entries (2^31 - 1 each)", rows, entries);
    begin_batch(s);
    const int bad = gfsmp::build_batch_matrix_form(cfg, nMol, nVertices, adj, feature, &s->lay);
    if (bad >= 0)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_prepare: molecule %d has max_nVertices = %d vertices and a vertex that reaches fewer than nNeighbors = %d "
                                         "of them: LCNN pads its sequence with row %d, past its matrix", bad, cfg.max_nVertices, cfg.nNeighbors,
                    cfg.max_nVertices);
    s->lv.assign(cfg.nLevels + 1, DevLevel());
    Taker t = {s};
    put_row_lists(t, lcnn);
    const size_t wgrad_ws = lcnn ? alloc_lcnn(t, (size_t)rows, nMol) : alloc_gcn_mw(t, (size_t)rows, nMol);
    t.put(&s->x, s->lay.x);
    t.alloc(&s->yhat, (size_t)nMol);
    t.alloc(&s->dy, (size_t)nMol);
    t.put(&s->top_node_mol, s->lay.nb_vertex_mol);
    t.put(&s->mol_ptr, s->lay.mol_first_vertex);
    if (t.st != GF_OK) return t.st;
    // (the weight gradients' partial images; the dense layer's TN product grows the workspace for its own)
    return finish_batch(s, std::max<size_t>(1 << 20, wgrad_ws));
}

// ---- the covariant handles (CGCN_1D, CGCN_2D; smp_level_covariant.hip): the host builds x, the hop counts and the column lists with their
// transposes (gfsmp::build_batch_covariant); the device gets those and the two buffers the forward kernel leaves for the reverse ----
gf_status covariant_prepare(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &cfg = s->cfg;
    long long rows = 0;
    for (int m = 0; m < nMol; ++m) {
        const gf_status st = check_max_vertices(s, "gf_smp_prepare", m, nVertices[m]);
        if (st != GF_OK) return st;
        rows += nVertices[m];
    }
    const size_t M = (size_t)cfg.max_nVertices, L = (size_t)cfg.nLevels;
    if (rows > 0x7fffffffll || (unsigned long long)rows * M * (L + 1) > 0x7fffffffull)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare: a covariant batch of %lld vertices: (nLevels + 1) x vertices x max_nVertices activations "
                                             "must stay below 2^31", rows);
    begin_batch(s);
    gfsmp::build_batch_covariant(cfg, nMol, nVertices, adj, feature, &s->lay);
    const gfsmp::BatchLayout::NeighbourList &nl = s->lay.nb_lists[0];
    s->lv.assign(cfg.nLevels + 1, DevLevel());
    Taker t = {s};
    long long *ptr = nullptr, *tptr = nullptr;
    int *idx = nullptr, *tidx = nullptr;
    t.put(&ptr, nl.ptr);
    t.put(&idx, nl.idx);
    t.put(&tptr, nl.tptr);
    t.put(&tidx, nl.tidx);
    s->cov_ptr = ptr, s->cov_idx = idx, s->cov_tptr = tptr, s->cov_tidx = tidx;
    t.put(&s->cov_hop, s->lay.cov_hop);
    t.put(&s->x, s->lay.x);
    t.alloc(&s->cov_h, (size_t)rows * M * (L + 1));
    t.alloc(&s->cov_n, (size_t)rows * M * L);
    t.alloc(&s->cov_ds0, (size_t)rows);
    t.alloc(&s->g, (size_t)nMol * M);
    t.alloc(&s->yhat, (size_t)nMol);
    t.alloc(&s->dy, (size_t)nMol);
    t.put(&s->top_node_mol, s->lay.nb_vertex_mol);
    t.put(&s->mol_ptr, s->lay.mol_first_vertex);
    if (t.st != GF_OK) return t.st;
    return finish_batch(s, std::max<size_t>(1 << 20, smp_covariant_ws_bytes(nMol, param_count(cfg))));   // (the gradient's partial images)
}

// null arguments (`have_all` = every pointer given and the count in range) / every graph has 1 .. 4096 vertices, in the entry point's words.
// nV2: the Y graphs of gf_smp_prepare_pairs, which also come under max_nVertices here, before the batch is copied.
gf_status check_graph_sizes(const gf_smp *s, const char *who, bool have_all, int n, const int *nV1, const int *nV2 = nullptr) {
    if (n <= 0 || !have_all) return fail(s->ctx, GF_ERR_INVALID, "%s: bad argument", who);
    for (int i = 0; i < n; ++i)
        for (int side = 0; side < (nV2 ? 2 : 1); ++side) {
            const int V = side ? nV2[i] : nV1[i];
            char what[96];
            if (nV2) std::snprintf(what, sizeof what, "%s: graph %c of pair %d", who, side ? 'Y' : 'X', i);
            else std::snprintf(what, sizeof what, "molecule %d", i);
            if (V <= 0 || V > 4096) return fail(s->ctx, GF_ERR_INVALID, "%s has %d vertices", what, V);
            if (nV2 && V > s->cfg.max_nVertices)
                return fail(s->ctx, GF_ERR_INVALID, "%s has %d vertices, the model was created with max_nVertices = %d", what, V, s->cfg.max_nVertices);
        }
    return GF_OK;
}

}  // namespace

// ints of a level's row-class buffer (see row_class_count), and its builder: three launches on `stream` behind whatever wrote trowf
// (live_only: a second set of block counts)
size_t smp_row_class_ints(int rows, bool live_only) {
    return 4 + 2 * ((size_t)rows + 64) + (live_only ? 2 : 1) * ((size_t)(rows + kRcBlock - 1) / kRcBlock + 1);
}
gf_status smp_build_row_classes(gf_ctx *ctx, hipStream_t stream, const int *trowf, int rows, int *buf, bool live_only) {
    if (rows < 1) return GF_OK;
    const int nb = (rows + kRcBlock - 1) / kRcBlock, lv = live_only ? 1 : 0;
    int *blockcnt = buf + 4 + 2 * ((size_t)rows + 64);
    hipLaunchKernelGGL(row_class_count, dim3(nb), dim3(kRcBlock), 0, stream, trowf, rows, blockcnt, lv);
    hipLaunchKernelGGL(row_class_scan, dim3(1), dim3(kRcBlock), 0, stream, blockcnt, nb, rows, buf, lv);
    hipLaunchKernelGGL(row_class_fill, dim3(nb), dim3(kRcBlock), 0, stream, trowf, rows, blockcnt, buf, reinterpret_cast<int2 *>(buf + 4), lv);
    GF_LAUNCH_CHECK(ctx, "row_class_fill");
    return GF_OK;
}
gf_status smp_build_row_class_nodes(gf_ctx *ctx, hipStream_t stream, const int *buf, int rows, const long long *node_row, int nodes, int *ent_node) {
    if (rows < 1 || nodes < 1) return GF_OK;
    hipLaunchKernelGGL(row_class_nodes, dim3((unsigned)((rows + 64 + 255) / 256)), dim3(256), 0, stream, buf, reinterpret_cast<const int2 *>(buf + 4), node_row,
                       nodes, ent_node);
    GF_LAUNCH_CHECK(ctx, "row_class_nodes");
    return GF_OK;
}
}  // namespace gf

using gf::fail;

extern "C" {

gf_status gf_smp_prepare(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature) {
    return gf_smp_prepare_coulomb(s, nMol, nVertices, adj, feature, nullptr);
}

gf_status gf_smp_prepare_coulomb(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature,
                                 const double *coulomb) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    gf_status st = gf::check_graph_sizes(s, "gf_smp_prepare", nVertices && adj && feature, nMol, nVertices);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->cfg.distance_channel)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_prepare: a distance handle (distance_channel = 1) takes its molecules through gf_smp_prepare_distance");
    if (s->cfg.readout == 1)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_prepare: a pair handle (readout = 1) takes its graphs through gf_smp_prepare_pairs");
    if ((s->cfg.steerable_2d || s->cfg.unrestricted || s->cfg.neighbourhood) && coulomb)   // (these classes have no use_coulomb constructor: their adjacency is the molecule's)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare_coulomb: a steerable_2d, unrestricted or neighbourhood handle has no Coulomb adjacency");
    if (s->cfg.matrix_form && coulomb)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare_coulomb: a matrix-form handle (LCNN, GCN_MW) has no Coulomb adjacency");
    if (s->cfg.matrix_form) return gf::smp_matrix_form_prepare(s, nMol, nVertices, adj, feature);
    if (s->cfg.covariant && coulomb)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare_coulomb: a covariant handle (CGCN_1D, CGCN_2D) has no Coulomb adjacency");
    if (s->cfg.covariant) return gf::covariant_prepare(s, nMol, nVertices, adj, feature);
    if (s->cfg.neighbourhood) return gf::neighbourhood_prepare(s, nMol, nVertices, adj, feature, nullptr);
    if (s->cfg.per_size()) return gf::smp_theta_prepare(s, nMol, nVertices, adj, feature);   // (first order: no reduced adjacency, coulomb is inert)
    st = gf::choose_plan(s, nMol, nVertices, adj, coulomb);
    if (st != GF_OK) return st;
    const bool prep_timing = std::getenv("GF_PREP_TIMING") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    gf::begin_batch(s);
    const auto tp1 = std::chrono::steady_clock::now();
    gf::choose_table_builder(s, nMol, nVertices);
    gfsmp::build_batch(s->cfg, nMol, nVertices, adj, feature, coulomb, &s->lay);
    const auto tp2 = std::chrono::steady_clock::now();
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 layout");
    const int L = s->cfg.nLevels, C = s->cfg.nChanels;
    s->lv.assign(L + 1, gf_smp::DevLevel());
    long long maxp = 0;
    size_t contract_ws = 0;
    for (int l = 0; l <= L && st == GF_OK; ++l) st = gf::alloc_level(s, l, &maxp, &contract_ws);
    if (st == GF_OK && s->lay.device_tables) st = gf::build_device_tables(s, coulomb != nullptr);
    if (st == GF_OK) st = gf::build_row_tables(s);
    // P [max ppos][C of the level below]: by far the largest buffer of the op-by-op path, taken from the pool only when a level needs it (ensure_P)
    s->P_count = (size_t)maxp;
    if (st == GF_OK) st = gf::alloc_readout(s, nMol);
    if (st != GF_OK) return st;
    // split-K partials of the weight gradients also live in the context workspace
    const size_t gemm_ws = sizeof(float) * 4400 * (size_t)4 * C * C + sizeof(float) * 4400 * (size_t)C * s->cfg.fdim() + (1 << 20);
    st = gf::finish_batch(s, std::max(contract_ws, gemm_ws));
    if (st == GF_OK && prep_timing) {
        const auto tp3 = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        std::fprintf(stderr, "gf_smp_prepare: release %.1f ms, host graph preparation %.1f ms, device allocation + upload %.1f ms\n",
                     ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3));
    }
    return st;
}

gf_status gf_smp_prepare_distance(gf_smp *s, int nMol, const int *nVertices, const int *adj, const double *feature, const double *distance) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (s->cfg.readout == 1)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_prepare_distance: a pair handle (readout = 1) takes its graphs through gf_smp_prepare_pairs");
    if (!s->cfg.distance_channel)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare_distance: the handle has no distance channel (gf_smp_config.distance_channel = 0)");
    const gf_status st = gf::check_graph_sizes(s, "gf_smp_prepare_distance", nVertices && adj && feature && distance, nMol, nVertices);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return gf::neighbourhood_prepare(s, nMol, nVertices, adj, feature, distance);
}

gf_status gf_smp_prepare_pairs(gf_smp *s, int nPairs, const int *nVertices1, const int *adj1, const double *feature1, const int *nVertices2,
                               const int *adj2, const double *feature2) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (s->cfg.readout != 1)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_prepare_pairs: the handle has no pair read-out (gf_smp_config.readout = %d)", s->cfg.readout);
    const bool have_all = nPairs <= 0x3fffffff && nVertices1 && adj1 && feature1 && nVertices2 && adj2 && feature2;
    const gf_status st = gf::check_graph_sizes(s, "gf_smp_prepare_pairs", have_all, nPairs, nVertices1, nVertices2);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    gfsmp::PairBatch pb;   // the 2 nPairs graphs X_0, Y_0, X_1, Y_1, .. as one neighbourhood batch
    gfsmp::interleave_pairs(s->cfg.nFeatures, nPairs, nVertices1, adj1, feature1, nVertices2, adj2, feature2, &pb);
    return gf::neighbourhood_prepare(s, 2 * nPairs, pb.nVertices.data(), pb.adj.data(), pb.feature.data(), nullptr);
}

/* Host only: one molecule of a matrix-form configuration as gf_smp_prepare derives it -- LCNN's order and sequence, GCN_MW's A-hat. */
gf_status gf_smp_matrix_form_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature, int *order, int *sequence,
                                           double *norm_adj) {
    if (!cfg || !adj || !feature) return fail(nullptr, GF_ERR_INVALID, "gf_smp_matrix_form_molecule_host: bad argument");
    gfsmp::Config c;
    char why[640];
    const gf_status verdict = gfsmp::resolve_config(cfg, gfsmp::kHandleEntry, &c, why, sizeof why);
    if (verdict != GF_OK) return fail(nullptr, verdict, "%s", why);
    if (!c.matrix_form) return fail(nullptr, GF_ERR_INVALID, "gf_smp_matrix_form_molecule_host: matrix_form = 0 is no matrix-form model");
    if (V < 1 || V > c.max_nVertices)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_matrix_form_molecule_host: %d vertices, the configuration has max_nVertices = %d", V, c.max_nVertices);
    if (c.matrix_form == 1 ? !order || !sequence : !norm_adj) return fail(nullptr, GF_ERR_INVALID, "gf_smp_matrix_form_molecule_host: missing output");
    gfsmp::MatrixFormMolecule m;
    gfsmp::matrix_form_molecule(c, V, adj, feature, &m);
    if (c.matrix_form == 2) {
        for (size_t i = 0; i < m.norm_adj.size(); ++i) norm_adj[i] = m.norm_adj[i];
        return GF_OK;
    }
    if (gfsmp::lcnn_reads_past(c, V, m.seq))
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_matrix_form_molecule_host: the molecule has max_nVertices = %d vertices and a vertex that reaches fewer "
                                             "than nNeighbors = %d of them: LCNN pads its sequence with row %d, past its matrix", V, c.nNeighbors, V);
    for (size_t i = 0; i < m.order.size(); ++i) order[i] = m.order[i];
    for (size_t i = 0; i < m.seq.size(); ++i) sequence[i] = m.seq[i];
    return GF_OK;
}

/* Host only: one molecule of a covariant configuration (CGCN_1D, CGCN_2D) as gf_smp_prepare derives it -- lists [V][M + 1] (slot 0 = the
 * size of N(v), then its members, -1 behind them), hop [V][M] (hop[v][i] = sp[i][v], 255 = unreachable or beyond the molecule) and,
 * optionally, x [V][F (D + 1)]. */
gf_status gf_smp_covariant_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature, int *lists, unsigned char *hop,
                                         double *x) {
    if (!cfg || !adj || !feature || !lists || !hop) return fail(nullptr, GF_ERR_INVALID, "gf_smp_covariant_molecule_host: bad argument");
    gfsmp::Config c;
    char why[640];
    const gf_status verdict = gfsmp::resolve_config(cfg, gfsmp::kHandleEntry, &c, why, sizeof why);
    if (verdict != GF_OK) return fail(nullptr, verdict, "%s", why);
    if (!c.covariant) return fail(nullptr, GF_ERR_INVALID, "gf_smp_covariant_molecule_host: covariant = 0 is no covariant model");
    if (V < 1 || V > c.max_nVertices)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_covariant_molecule_host: %d vertices, the configuration has max_nVertices = %d", V, c.max_nVertices);
    gfsmp::BatchLayout B;
    gfsmp::build_batch_covariant(c, 1, &V, adj, feature, &B);
    const int M = c.max_nVertices;
    const gfsmp::BatchLayout::NeighbourList &nl = B.nb_lists[0];
    for (int v = 0; v < V; ++v) {
        int *row = lists + (size_t)v * (M + 1);
        const long long e0 = nl.ptr[(size_t)v], n = nl.ptr[(size_t)v + 1] - e0;
        row[0] = (int)n;
        for (int i = 0; i < M; ++i) row[1 + i] = i < n ? nl.idx[(size_t)(e0 + i)] : -1;
    }
    for (size_t i = 0; i < (size_t)V * M; ++i) hop[i] = B.cov_hop[i];
    if (x)
        for (size_t i = 0; i < B.mols[0].wl.size(); ++i) x[i] = B.mols[0].wl[i];
    return GF_OK;
}

/* Host-only graph preparation of ONE molecule (no device needed): receptive fields phi[l][v] as
 * [L+1][V][cap+1] ints (slot 0 = size) and, optionally, the WL features [V][F(D+1)].  Lets the host logic be tested
 * on a CPU-only box and inspected by callers. */
gf_status gf_smp_prepare_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature,
                                       int *phi_out, double *wl_out) {
    if (!cfg || V <= 0 || !adj || !feature || !phi_out) return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: bad argument");
    // The families without a cap: a configuration no handle or tower is built from is not one of theirs (gfsmp::resolve_config's verdict, asked
    // as a tower -- the widest entry; the family named is the one it judged).  Everything else is prepared as it stands.
    gfsmp::Config resolved;
    char why[640];
    const bool refused = gfsmp::resolve_config(cfg, {gfsmp::ConfigEntry::Tower, 0, 0.0}, &resolved, why, sizeof why) != GF_OK;
    if (cfg->matrix_form)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: a matrix-form model (LCNN, GCN_MW) has no receptive fields: "
                                             "gf_smp_matrix_form_molecule_host");
    if (cfg->covariant)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: a covariant model (CGCN_1D, CGCN_2D) has masks, not capped receptive "
                                             "fields: gf_smp_covariant_molecule_host");
    if (cfg->neighbourhood)   // (about this call, not the configuration)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: a neighbourhood model (NeuralFingerprint, GCN_1D, GCN_2D) has no receptive fields");
    if (refused && cfg->unrestricted)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: unrestricted = %d needs first_order = steerable_2d = 0 and max_receptive_field "
                                             "== max_nVertices", cfg->unrestricted);
    if (refused && cfg->steerable_2d)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: steerable_2d = %d needs first_order = 0 and max_receptive_field == max_nVertices",
                    cfg->steerable_2d);
    if (refused && cfg->first_order >= 2)   // (SMP_1D* have no cap: a capped field is not one of theirs)
        return fail(nullptr, GF_ERR_INVALID, "gf_smp_prepare_molecule_host: first_order = %d needs max_receptive_field == max_nVertices", cfg->first_order);
    gfsmp::Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, cfg->has_WL_ordering};
    c.physics = cfg->physics ? 1 : 0;
    gfsmp::Molecule m;
    gfsmp::prepare_molecule(c, V, adj, feature, &m);
    const int cap = c.max_receptive_field;
    for (int l = 0; l <= c.nLevels; ++l)
        for (int v = 0; v < V; ++v) {
            int *p = phi_out + ((size_t)l * V + v) * (cap + 1);
            const std::vector<int> &f = m.phi[l][v];
            p[0] = (int)f.size();
            for (int i = 0; i < cap; ++i) p[1 + i] = i < (int)f.size() ? f[i] : -1;
        }
    if (wl_out)
        for (size_t i = 0; i < m.wl.size(); ++i) wl_out[i] = m.wl[i];
    return GF_OK;
}

}  // extern "C"
