// genome_edits.h -- what polish_genome.hip (every single-letter edit) and polish_variants.hip (proposed variants of any length) share:
// a checked window of the packed genome, an edit of it as the replacement of nd letters at u by m letters, the (start, ndel, new
// symbols) of that edit as bio.edit_states gives them for the spelled-out strings, and the small pieces of the two sum kernels
// (design/polish_genome.md 1, design/polish_variants.md 1.3).  The base digit and the complement are also genome_map.hip's and
// align.hip's.
//
// Every input is device data and is NOT trusted: no loop bound and no address depends on a value that has not been checked in the
// same kernel.
#pragma once
#include "common.h"

#define GE_WAVES 4
#define GE_THREADS 256
#define GE_NONE (-1)

typedef unsigned long long u64;

__device__ __forceinline__ int ge_digit(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
__device__ __forceinline__ int ge_comp(int c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// ---- windows -------------------------------------------------------------------------------------------------------------------------

struct ge_win {
    const uint8_t *g;          // the window's first forward letter
    long long off, w0, w1;     // the packed position of its contig, and [w0, w1) within it
    int n;                     // letters
    bool rev;
    __device__ __forceinline__ int at(int u) const { return rev ? ge_comp(g[n - 1 - u]) : (int)g[u]; }
};

// A window's span, checked: -> letters, or -1 when it is no span of the genome the kernels take.
__device__ __forceinline__ long long ge_window_len(long long off, long long w0, long long w1, long long G)
{
    if (off < 0 || w0 < 0 || w1 < w0 || off > G || w1 > G - off || w1 - w0 > 0x7ffffff0ll) return -1;
    return w1 - w0;
}

// minus == nullptr: the forward strand
__device__ __forceinline__ bool ge_open(const uint8_t *__restrict__ genome, const int64_t *__restrict__ win_off,
                                        const int64_t *__restrict__ w0, const int64_t *__restrict__ w1,
                                        const int32_t *__restrict__ minus, int b, long long G, ge_win *w)
{
    const long long off = win_off[b], a = w0[b], e = w1[b], n = ge_window_len(off, a, e, G);
    if (n < 0) return false;
    w->g = genome + off + a;
    w->off = off;
    w->w0 = a;
    w->w1 = e;
    w->n = (int)n;
    w->rev = minus ? minus[b] != 0 : false;
    return true;
}

// the entry of an ascending table off[0 .. n] that holds i: the last b in [0, n) with off[b] <= i (0 when there is none)
__device__ __forceinline__ int ge_find(const int64_t *__restrict__ off, int n, long long i)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// the posterior column of the k-mer of `klen` letters read through `at`; -1 when a letter is none of A C G T
template <typename F>
__device__ __forceinline__ int ge_column(F at, int first, int klen, int blank)
{
    int s = 0;
    bool bad = false;
    for (int d = 0; d < klen; d++) {
        const int x = ge_digit(at(first + d));
        bad |= x < 0;
        s = s * 4 + (x & 3);
    }
    return bad ? -1 : s + (s >= blank ? 1 : 0);
}

// ---- edits ---------------------------------------------------------------------------------------------------------------------------
// An edit E of a window's string s: s' = s[:u] + new + s[u + nd:], with members u, nd, m and letter(x), letter x of the m new ones
// on the window's strand.  A single letter is (nd, m) = substitution (1, 1), deletion (1, 0), insertion (0, 1).

// letter i of the edited string
template <typename E>
__device__ __forceinline__ int ge_edited_at(const ge_win &w, const E &e, int i)
{
    return i < e.u ? w.at(i) : i < e.u + e.m ? e.letter(i - e.u) : w.at(i - e.m + e.nd);
}

// (start, ndel, number of new k-mers) of bio.edit_states for the window's string and its edit: the common prefix of the two k-mer
// lists first, then the common suffix of the rest.  dF: the first letter at which the strings differ read from the front, dB: the
// last letter of the OLD string at which they differ read from the back (GE_NONE: they agree as far as the shorter goes).  Both
// searches start at the edit (the strings agree outside it by construction), run on along a repeat and end at the window's ends at
// the latest.
template <typename E>
__device__ __forceinline__ void ge_triple(const ge_win &w, const E &e, int klen, int *start, int *ndel, int *nnew)
{
    const int n = w.n, n2 = n - e.nd + e.m, mn = n < n2 ? n : n2;
    int i = e.u;
    while (i < mn && w.at(i) == ge_edited_at(w, e, i)) i++;
    const int dF = i < mn ? i : GE_NONE;
    int t = n - e.u - e.nd;                                      // the letters behind the edit, equal in both
    while (t < mn && w.at(n - 1 - t) == ge_edited_at(w, e, n2 - 1 - t)) t++;
    const int dB = t < mn ? n - 1 - t : GE_NONE;
    const int nold = n - klen + 1, nnw = n2 - klen + 1, nmin = nold < nnw ? nold : nnw;
    int pre = nmin;
    if (dF != GE_NONE) {
        pre = dF - klen + 1 > 0 ? dF - klen + 1 : 0;
        if (pre > nmin) pre = nmin;
    }
    const int rest = nmin - pre;
    int suf = rest;
    if (dB != GE_NONE) {
        suf = nold - 1 - dB > 0 ? nold - 1 - dB : 0;
        if (suf > rest) suf = rest;
    }
    *start = pre;
    *ndel = nold - pre - suf;
    *nnew = nnw - pre - suf;
}

// A candidate's new symbols: the columns of the edited string's k-mers from `start` on, written to its slice [new_off[0], new_off[1])
// of cand_new when the slice lies inside the new_cap symbols there are, has at most max_new of them and ends inside the string.
template <typename E>
__device__ __forceinline__ void ge_write_new(const ge_win &w, const E &e, int klen, int blank, int start,
                                             const int64_t *__restrict__ new_off, long long new_cap, int max_new,
                                             int32_t *__restrict__ cand_new)
{
    const long long a = new_off[0], m = new_off[1] - a;
    const int n2 = w.n - e.nd + e.m;
    if (start < 0 || m < 0 || m > max_new || a < 0 || a + m > new_cap || start + m + klen - 1 > n2) return;
    for (int x = 0; x < (int)m; x++)
        cand_new[a + x] = ge_column([&](int j) { return ge_edited_at(w, e, j); }, start + x, klen, blank);
}

// ---- the sorted candidate list of the sum kernels ------------------------------------------------------------------------------------

// an entry c of `order` (the host's sort, device data): does it name one of the ncand candidates?
__device__ __forceinline__ bool ge_listed(long long c, long long ncand) { return c >= 0 && c < ncand; }

// is entry i, whose candidate has key k, the first of its segment of equal keys?
template <typename K>
__device__ __forceinline__ bool ge_segment_head(const int64_t *__restrict__ order, long long ncand, long long i,
                                                const K *__restrict__ key, K k)
{
    if (i == 0) return true;
    const long long cp = order[i - 1];
    return !(ge_listed(cp, ncand) && key[cp] == k);
}

// a candidate's value l and its read's score s: either is a NaN (a refused candidate or pair), both are finite, or neither
enum { GE_PAIR_NAN, GE_PAIR_FINITE, GE_PAIR_NEITHER };
__device__ __forceinline__ int ge_classify(double l, double s)
{
    return l != l || s != s ? GE_PAIR_NAN : l - l == 0.0 && s - s == 0.0 ? GE_PAIR_FINITE : GE_PAIR_NEITHER;
}

// ---- the entries' screens ------------------------------------------------------------------------------------------------------------

static inline unsigned ge_blocks(long long n) { return (unsigned)((n + GE_THREADS - 1) / GE_THREADS); }

static inline bool ge_klen(int klen) { return klen >= 3 && klen <= SLK_RESCORE_MAX_NEW - 1; }
