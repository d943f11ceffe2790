// genome_map.hip -- where on a genome a called read lies: k-mer keys of the genome, a seed-and-vote stage over diagonals, and the
// cut of genome spans on either strand (row f7, design/genome_map.md).
//
// Stands for the locating half of misc/align.py:46-67 (`bwa mem -k14 ... genome.fa calls.fa`: the aligner is handed a GENOME, not a
// reference per read) and for the cut of misc/get_refs_from_sam.py:40-68 (one padded, strand-corrected reference per read).  The
// scoring half is csrc/align.hip, used as it is: this file only chooses, per read, a window of the genome for it.
//
// Letters are bytes; A C G T = 0..3 and any other byte breaks every k-mer that contains it.  A k-mer's code is the base-4 number of
// its letters, first letter most significant (the rule of csrc/bases.hip), k = 8..15, so a code is below 2^30.
//
//   keys   key[p] = code(p) << 32 | p for every genome position p; a k-mer that holds another byte, crosses its contig's end or the
//          genome's gets the code field 0x7FFFFFFF and sorts behind every real one.  The caller sorts the keys (they are distinct,
//          so the order is unique and positions ascend within a code).  There is no 4^k table: lookups search the sorted keys.
//   votes  one workgroup works on one (query, strand) at a time.  For query position i with a valid k-mer: its range in the sorted
//          keys (skipped when it has more than max_occ entries), and for every occurrence p the diagonal D = p - i + 65536, counted
//          in the bins D / W and D / W - 1: bin b covers the diagonals [b W, (b + 2) W), the bins half overlap.  The '-' strand is
//          the reverse complement of the query against the forward genome: the k-mer at i of the query is, complemented and read
//          backwards, the k-mer at n - k - i of the reverse complement, so both strands read the same letters.
//          The counts are int32 in a slab of the workspace that belongs to the workgroup: it zeroes the slab once, counts with
//          integer atomics whose RETURN values give the greatest count and its smallest bin, and in a second walk over the same
//          occurrences exchanges every count it touched for 0 (the first exchange of a bin returns its count, later ones 0), which
//          yields `second` and leaves the slab zero for the workgroup's next item.  Integer sums do not depend on the order of
//          arrival, so no result depends on scheduling; nothing waits on another workgroup.
//   windows  out[out_off[b] + j] = genome[start[b] + j], or complement(genome[end[b] - 1 - j]) for a '-' span (the complement of
//          slk_revcomp_u8: A<->T, C<->G, every other byte unchanged).
#include "genome_edits.h"                       // the base digit and the complement

#define GM_THREADS 256
#define GM_MIN_K 8
#define GM_MAX_K 15
#define GM_INVALID 0x7FFFFFFF
#define GM_DIAG0 65536                         // added to p - i: keeps a diagonal positive and the bins independent of the batch
#define GM_MAX_QLEN 65535
#define GM_MAX_OCC 4096                        // 65535 positions * 4096 occurrences * 2 bins < 2^31: no count overflows
#define GM_MAX_GROUPS 2048
#define GM_WORKSPACE_CAP ((size_t)4 << 30)

__global__ void __launch_bounds__(GM_THREADS) genome_keys_kernel(const uint8_t *__restrict__ genome,
                                                                 const int64_t *__restrict__ contig_off, int ncontig, long long G,
                                                                 int k, int64_t *__restrict__ keys, int32_t *__restrict__ nvalid)
{
    const long long p = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
    bool valid = false;
    if (p < G) {
        int lo = 1, hi = ncontig;                                // the first c in 1..ncontig with contig_off[c] > p: p's contig ends there
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (contig_off[mid] > p) hi = mid; else lo = mid + 1;
        }
        valid = p + k <= contig_off[lo];
        unsigned code = 0;
        if (valid)
            for (int j = 0; j < k; j++) {
                const int l = ge_digit(genome[p + j]);
                valid &= l >= 0;
                code = (code << 2) | (unsigned)(l & 3);
            }
        keys[p] = (int64_t)(((u64)(valid ? code : (unsigned)GM_INVALID) << 32) | (u64)p);
    }
    const u64 m = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(nvalid, (int)__popcll(m));      // an integer count: the order cannot matter
}

// greatest value over the workgroup, in every thread (two barriers: the scratch may be reused at once)
__device__ __forceinline__ u64 gm_block_max(u64 v, u64 *scratch)
{
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
        const u64 o = ((u64)(unsigned)__shfl_xor((int)(v >> 32), mask) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, mask);
        if (o > v) v = o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = scratch[0];
#pragma unroll
    for (int w = 1; w < GM_THREADS / 64; w++) r = scratch[w] > r ? scratch[w] : r;
    return r;
}

__device__ __forceinline__ int gm_block_sum(int v, int *scratch)
{
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < GM_THREADS / 64; w++) r += scratch[w];
    return r;
}

__global__ void __launch_bounds__(GM_THREADS) genome_seed_kernel(const uint8_t *__restrict__ q, long ldq,
                                                                 const int32_t *__restrict__ qlen, int B, int max_qlen,
                                                                 const int64_t *__restrict__ keys, int nvalid, int k, int logw,
                                                                 int max_occ, int nbins, int32_t *__restrict__ out,
                                                                 int32_t *__restrict__ workspace, size_t group_ints, int row_ints)
{
    __shared__ u64 smax[GM_THREADS / 64];
    __shared__ int ssum[GM_THREADS / 64];
    const int tid = threadIdx.x;
    int32_t *cnt = workspace + (size_t)blockIdx.x * group_ints;  // [nbins] counts, then per query position the range it found
    int32_t *first = cnt + (group_ints - 2 * (size_t)row_ints), *nocc = first + row_ints;
    for (int j = tid; j < nbins; j += GM_THREADS) cnt[j] = 0;
    __threadfence();                                             // the zeroes are in memory before any atomic of this workgroup
    __syncthreads();

    for (int item = blockIdx.x; item < 2 * B; item += gridDim.x) {
        const int b = item >> 1, minus = item & 1;
        const int n = qlen[b];
        int32_t *o = out + (size_t)item * 4;
        if (n < 0 || n > max_qlen) {                             // refused, never truncated (uniform over the workgroup)
            if (tid < 4) o[tid] = tid == 0 ? -1 : 0;
            continue;
        }
        const uint8_t *qb = q + (size_t)b * ldq;
        const int npos = n - k + 1;
        u64 best = 0;                                            // count:32 | ~bin:32 -> greatest count, then smallest bin
        int nseed = 0;
        for (int i = tid; i < npos; i += GM_THREADS) {
            unsigned fwd = 0, rev = 0;
            bool ok = true;
            for (int j = 0; j < k; j++) {
                const int l = ge_digit(qb[i + j]);
                ok &= l >= 0;
                fwd = (fwd << 2) | (unsigned)(l & 3);
                rev |= (unsigned)(3 - (l & 3)) << (2 * j);
            }
            const unsigned code = minus ? rev : fwd;
            const int qi = minus ? n - k - i : i;                // the k-mer's position in the sequence that is being placed
            int lo = 0, found = 0;
            if (ok) {
                int hi = nvalid;
                const int64_t target = (int64_t)((u64)code << 32);
                while (lo < hi) {
                    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                    if (keys[mid] < target) lo = mid + 1; else hi = mid;
                }
                const bool skip = (long long)lo + max_occ < nvalid && (unsigned)(keys[lo + max_occ] >> 32) == code;
                if (!skip) {
                    nseed++;
                    for (; found < max_occ && lo + found < nvalid; found++) {
                        const int64_t key = keys[lo + found];
                        if ((unsigned)(key >> 32) != code) break;
                        const int bin = (int)(((unsigned)key - (unsigned)qi + (unsigned)GM_DIAG0) >> logw);
                        if (bin < 1 || bin >= nbins) continue;   // (keys that were not made from this genome: never out of the slab)
                        const unsigned c1 = (unsigned)atomicAdd(&cnt[bin], 1) + 1u, c0 = (unsigned)atomicAdd(&cnt[bin - 1], 1) + 1u;
                        const u64 k1 = ((u64)c1 << 32) | (0xffffffffu - (unsigned)bin);
                        const u64 k0 = ((u64)c0 << 32) | (0xffffffffu - (unsigned)(bin - 1));
                        best = k1 > best ? k1 : best;
                        best = k0 > best ? k0 : best;
                    }
                }
            }
            first[i] = lo;
            nocc[i] = found;
        }
        best = gm_block_max(best, smax);                         // (its barriers: every count of the item is final behind them)
        nseed = gm_block_sum(nseed, ssum);
        const int votes = (int)(best >> 32), wbin = votes ? (int)(0xffffffffu - (unsigned)best) : 0;
        u64 second = 0;
        for (int i = tid; i < npos; i += GM_THREADS) {           // the same thread wrote first[i] / nocc[i]
            const int lo = first[i], cntocc = nocc[i];
            const int qi = minus ? n - k - i : i;
            for (int j = 0; j < cntocc; j++) {
                const int bin = (int)(((unsigned)keys[lo + j] - (unsigned)qi + (unsigned)GM_DIAG0) >> logw);
                if (bin < 1 || bin >= nbins) continue;
                const unsigned c1 = (unsigned)atomicExch(&cnt[bin], 0), c0 = (unsigned)atomicExch(&cnt[bin - 1], 0);
                if ((bin > wbin ? bin - wbin : wbin - bin) > 2 && c1 > second) second = c1;
                if ((bin - 1 > wbin ? bin - 1 - wbin : wbin - (bin - 1)) > 2 && c0 > second) second = c0;
            }
        }
        second = gm_block_max(second, smax);                     // (its barriers: the slab is zero again behind them)
        if (tid == 0) {
            o[0] = wbin;
            o[1] = votes;
            o[2] = (int)second;
            o[3] = nseed;
        }
    }
}

__global__ void __launch_bounds__(256) genome_windows_kernel(const uint8_t *__restrict__ genome, long long G,
                                                             const int64_t *__restrict__ start, const int64_t *__restrict__ end,
                                                             const int32_t *__restrict__ minus, const int64_t *__restrict__ out_off,
                                                             uint8_t *__restrict__ out)
{
    const long long s = start[blockIdx.x], e = end[blockIdx.x], o = out_off[blockIdx.x];
    if (s < 0 || e > G || e < s || e - s != out_off[blockIdx.x + 1] - o) return;         // not a span of this genome: nothing is read
    const bool rc = minus[blockIdx.x] != 0;
    for (long long j = (long long)blockIdx.y * 256 + threadIdx.x; j < e - s; j += (long long)gridDim.y * 256) {
        const uint8_t c = rc ? genome[e - 1 - j] : genome[s + j];
        out[o + j] = rc ? (uint8_t)ge_comp(c) : c;
    }
}

extern "C" int slk_genome_kmer_keys_u8(const uint8_t *genome, const int64_t *contig_off, int ncontig, long G, int k, int64_t *keys,
                                       int32_t *nvalid, slk_stream_t stream)
{
    if (G < 0 || G >= (1L << 31) || ncontig < 1 || k < GM_MIN_K || k > GM_MAX_K || !nvalid) return SLK_ERR_INVALID_ARG;
    if (hipMemsetAsync(nvalid, 0, sizeof(int32_t), slk_stream(stream)) != hipSuccess) return SLK_ERR_LAUNCH;
    if (G == 0) return SLK_OK;
    if (!genome || !contig_off || !keys) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(genome_keys_kernel, dim3((unsigned)((G + GM_THREADS - 1) / GM_THREADS)), dim3(GM_THREADS), 0, slk_stream(stream),
                       genome, contig_off, ncontig, (long long)G, k, keys, nvalid);
    return slk_launch_status();
}

static int gm_log2(int w)
{
    int l = 0;
    while ((1 << l) < w) l++;
    return l;
}

static bool gm_seed_shape_ok(int B, int max_qlen, long G, int bin_width)
{
    return B >= 0 && max_qlen >= 0 && G >= 0 && G < (1L << 31) && bin_width >= 2 && bin_width <= 32768 &&
           (bin_width & (bin_width - 1)) == 0 && max_qlen + bin_width <= GM_DIAG0;       // so that D >= W: the lower bin is never -1
}

static size_t gm_row_ints(int max_qlen) { return ((size_t)(max_qlen > 0 ? max_qlen : 1) + 3) / 4 * 4; }

static size_t gm_group_ints(int max_qlen, long G, int bin_width)
{
    const size_t nbins = (size_t)((G + GM_DIAG0 - 1) >> gm_log2(bin_width)) + 1;
    return (nbins + 3) / 4 * 4 + 2 * gm_row_ints(max_qlen);
}

extern "C" size_t slk_genome_seed_workspace_bytes(int B, int max_qlen, long G, int bin_width)
{
    if (!gm_seed_shape_ok(B, max_qlen, G, bin_width) || B == 0) return 0;
    const size_t group = gm_group_ints(max_qlen, G, bin_width) * sizeof(int32_t);
    size_t groups = 2 * (size_t)B < GM_MAX_GROUPS ? 2 * (size_t)B : GM_MAX_GROUPS;
    if (groups * group > GM_WORKSPACE_CAP) groups = GM_WORKSPACE_CAP / group;
    return (groups ? groups : 1) * group;
}

extern "C" int slk_genome_seed_votes_u8(const uint8_t *q, long ldq, const int32_t *qlen, int B, int max_qlen, const int64_t *keys,
                                        int nvalid, long G, int k, int bin_width, int max_occ, int32_t *out, void *workspace,
                                        size_t workspace_bytes, slk_stream_t stream)
{
    if (!gm_seed_shape_ok(B, max_qlen, G, bin_width) || max_qlen > GM_MAX_QLEN || k < GM_MIN_K || k > GM_MAX_K || max_occ < 1 ||
        max_occ > GM_MAX_OCC || nvalid < 0 || nvalid > G)
        return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!q || !qlen || !out || (nvalid && !keys) || ldq < max_qlen) return SLK_ERR_INVALID_ARG;
    const size_t group = gm_group_ints(max_qlen, G, bin_width);
    if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < group * sizeof(int32_t)) return SLK_ERR_WORKSPACE;
    size_t groups = workspace_bytes / (group * sizeof(int32_t));
    if (groups > 2 * (size_t)B) groups = 2 * (size_t)B;
    if (groups > GM_MAX_GROUPS) groups = GM_MAX_GROUPS;
    const int logw = gm_log2(bin_width);
    hipLaunchKernelGGL(genome_seed_kernel, dim3((unsigned)groups), dim3(GM_THREADS), 0, slk_stream(stream), q, ldq, qlen, B, max_qlen,
                       keys, nvalid, k, logw, max_occ, (int)(((G + GM_DIAG0 - 1) >> logw) + 1), out, (int32_t *)workspace, group,
                       (int)gm_row_ints(max_qlen));
    return slk_launch_status();
}

extern "C" int slk_genome_windows_u8(const uint8_t *genome, long G, const int64_t *start, const int64_t *end, const int32_t *minus,
                                     const int64_t *out_off, int B, long max_len, uint8_t *out, slk_stream_t stream)
{
    if (B < 0 || max_len < 0 || G < 0) return SLK_ERR_INVALID_ARG;
    if (B == 0 || max_len == 0) return SLK_OK;
    if (!genome || !start || !end || !minus || !out_off || !out || out == genome) return SLK_ERR_INVALID_ARG;
    const long blocks = (max_len + 255) / 256;
    hipLaunchKernelGGL(genome_windows_kernel, dim3(B, (unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, slk_stream(stream), genome,
                       (long long)G, start, end, minus, out_off, out);
    return slk_launch_status();
}
