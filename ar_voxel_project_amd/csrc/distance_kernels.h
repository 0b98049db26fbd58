// distance_kernels.h -- the exact signed squared Euclidean distance field of the occupancy
// (arvx_distance) and the ball morphology that thresholds it (arvx_morph); definition in
// include/arvx/arvx.h, rationale in DESIGN.md 4.12.
//
// The field S is one int32 per voxel, flat index order, and is transformed IN PLACE by three passes.
// After the passes along x, x y and x y z it holds, for an occupied voxel, + the least squared
// distance to an empty site of the voxel's row, plane, grid, and for an empty voxel - the least squared
// distance to an occupied voxel of the same; +-kDistInf where there is no such site.  One signed value
// per voxel is enough at every stage because a voxel is a site of its own kind at distance 0: the
// partial distance to its own kind is always 0 and never has to be stored.
//
//   dist_row_kernel        pass 1, from the 64-bit words of the occupancy plane (bitplane_kernels.h):
//                          count trailing / leading zeros of the masked words, the neighbouring
//                          words of the row where the voxel's own word holds no opposite bit, the
//                          border sites x = -1 and x = X
//   dist_column_kernel     passes 2 and 3: per column min_j (f(j) + (y - j)^2) by the linear-time
//                          lower-envelope scan (Meijster et al. 2000; Felzenszwalb & Huttenlocher
//                          2012) in integers, a lane per column and sign, lanes along x; both signs in
//                          one launch, side by side
//   dist_threshold_kernel  the field against a squared radius -> one word of a bit plane per wave
//                          (ballot) and the number of its set bits
#pragma once

#include "bitplane_kernels.h"

namespace arvx {

constexpr int kDistInf = 2147483647;  // ARVX_DISTANCE_INF

// Words a wave of dist_row_kernel / dist_threshold_kernel handles one after the other: the word's row and
// place in it cost two 64-bit divisions, paid once per wave and counted up from there.
constexpr int kDistWordsPerWave = 8;

// lane `src`'s value of a 64-bit word (every lane of the wave takes part)
__device__ __forceinline__ unsigned long long dist_shfl64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// Pass 1.  A wave takes kDistWordsPerWave consecutive words of the plane; lane b is voxel x = 64 * xw + b
// of the word's row.  Where the voxel's own word holds no bit of the other kind the nearest word that
// does is the same for the whole wave: the lanes hold a window of 64 words of the row (one load), a
// ballot says which of them hold an occupied bit and which an empty one, and the word is fetched from
// its lane.  Rows of more than 64 words go on through memory where the window has no such word.
// Invariant: held[] and nz[] are those of (held_row, held_base), and everything up to `if (x < g.X)` is
// wave-uniform, so every lane of the wave reaches every ballot and shuffle.
__global__ __launch_bounds__(256) void dist_row_kernel(const unsigned long long *__restrict__ occ, const BitGrid g,
                                                       int border_empty, int *__restrict__ S) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    size_t wi = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kDistWordsPerWave;
    if (wi >= nwords) return;  // (the whole wave: every lane stays to the end)
    const int b = (int)(threadIdx.x & 63);
    int xw = (int)(wi % g.XW);
    size_t row = wi / g.XW;
    const int tail = g.X & 63;  // valid bits of a row's last word (0: all)
    // word k of the row as the bits of the voxels of one kind (kind 1: occupied, kind 0: empty)
    auto bits_of = [&](unsigned long long w, int k, int kind) -> unsigned long long {
        if (kind) return w;
        return (k == g.XW - 1 && tail) ? ~w & ((1ull << tail) - 1ull) : ~w;
    };
    size_t held_row = ~(size_t)0;
    int held_base = -1;
    unsigned long long held[2] = {0ull, 0ull}, nz[2] = {0ull, 0ull};  // [kind]; nz: the window's words with a bit
    for (int k8 = 0; k8 < kDistWordsPerWave && wi < nwords; ++k8, ++wi) {
        const unsigned long long *r = occ + row * g.XW;
        const int base = xw & ~63;
        if (row != held_row || base != held_base) {
            const int k = base + b;
            const unsigned long long w = k < g.XW ? r[k] : 0ull;
            held[1] = k < g.XW ? w : 0ull;
            held[0] = k < g.XW ? bits_of(w, k, 0) : 0ull;
            nz[0] = __ballot(held[0] != 0ull);
            nz[1] = __ballot(held[1] != 0ull);
            held_row = row;
            held_base = base;
        }
        // the nearest word beyond xw, on either side, with a bit of either kind: its place in the row
        // (-1: none) and the bits -- the same for every lane
        const int l = xw - base;
        int far_k[2][2];                 // [kind][0: towards smaller x, 1: towards larger x]
        unsigned long long far_w[2][2];
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            const unsigned long long up = nz[kind] & ~(((1ull << l) << 1) - 1ull), down = nz[kind] & ((1ull << l) - 1ull);
            int ku = up ? base + (__ffsll((long long)up) - 1) : -1;
            int kd = down ? base + (63 - __clzll((long long)down)) : -1;
            unsigned long long wu = dist_shfl64(held[kind], up ? ku - base : 0);
            unsigned long long wd = dist_shfl64(held[kind], down ? kd - base : 0);
            if (ku < 0) {  // (rows of more than 64 words)
                wu = 0ull;
                for (int k = base + 64; k < g.XW && !wu; ++k) {
                    wu = bits_of(r[k], k, kind);
                    ku = k;
                }
                if (!wu) ku = -1;
            }
            if (kd < 0) {
                wd = 0ull;
                for (int k = base - 1; k >= 0 && !wd; --k) {
                    wd = bits_of(r[k], k, kind);
                    kd = k;
                }
                if (!wd) kd = -1;
            }
            far_k[kind][1] = ku;
            far_w[kind][1] = wu;
            far_k[kind][0] = kd;
            far_w[kind][0] = wd;
        }
        const unsigned long long own1 = dist_shfl64(held[1], l), own0 = dist_shfl64(held[0], l);
        const int x = 64 * xw + b;
        if (x < g.X) {
            const bool occupied = (own1 >> b) & 1ull;
            const int other = occupied ? 0 : 1;                   // the kind this voxel looks for
            const unsigned long long own = occupied ? own0 : own1;  // ... and its bits in the voxel's own word
            int best = -1;  // distance along the row to the nearest opposite site (-1: none)
            {   // towards larger x
                const unsigned long long m = own & ~(((1ull << b) << 1) - 1ull);  // (bits above b; b = 63: none)
                const int k = other ? far_k[1][1] : far_k[0][1];
                const unsigned long long w = other ? far_w[1][1] : far_w[0][1];
                if (m) best = (__ffsll((long long)m) - 1) - b;
                else if (k >= 0) best = 64 * (k - xw) + (__ffsll((long long)w) - 1) - b;
                else if (occupied && border_empty) best = g.X - x;
            }
            {   // towards smaller x
                const unsigned long long m = own & ((1ull << b) - 1ull);
                const int k = other ? far_k[1][0] : far_k[0][0];
                const unsigned long long w = other ? far_w[1][0] : far_w[0][0];
                int d = -1;
                if (m) d = b - (63 - __clzll((long long)m));
                else if (k >= 0) d = b + 64 * (xw - k) - (63 - __clzll((long long)w));
                else if (occupied && border_empty) d = x + 1;
                if (d >= 0 && (best < 0 || d < best)) best = d;
            }
            const int v = best < 0 ? kDistInf : best * best;  // (best <= 46340: the square fits)
            S[row * (size_t)g.X + x] = occupied ? v : -v;
        }
        if (++xw == g.XW) {
            xw = 0;
            ++row;
        }
    }
}

// floor(n / d) for |n| < 2^33 and 0 < d < 2^17: the fp64 quotient is exact where n / d is an integer and
// further from every integer than its rounding error where it is not, so its floor is the answer; one
// step either way is still taken where the remainder says so.
__device__ __forceinline__ long long dist_floor_div(long long n, int d) {
    long long q = (long long)floor((double)n / (double)d);
    const long long r = n - q * d;
    if (r < 0) --q;
    else if (r >= d) ++q;
    return q;
}

// Passes 2 and 3.  Column c holds the `len` values S[base(c) + j * stride], base(c) = (c / X) * outer + c % X.
// A lane takes one column and one SIGN, consecutive lanes consecutive x: lanes [0, ncols) are sign 0,
// lanes [ncols, 2 ncols) sign 1.
//   sign 0: the envelope of the EMPTY sites (f = 0 at an empty voxel and at the border, the partial
//           distance at an occupied one), read back at the occupied voxels;
//   sign 1: the envelope of the OCCUPIED sites, read back at the empty voxels.
// The two lanes of a column run side by side on the same values: each writes the voxels of its own
// kind only and keeps their sign, and reads of the other kind's voxels nothing but the sign (f = 0
// there), so neither sees anything the other could change under it.  This is deliberate, and formally
// a race on plain accesses: it rests on the sign of a value never changing (a result is >= 1 in
// magnitude) and on aligned 32-bit loads and stores not tearing.  Do not widen these accesses into
// vector loads that span several voxels' values with other semantics, and do not "fix" it with atomics.
// Sites: coordinate j in [-1, len], the two ends being the border's empty sites.  The envelope is a
// stack of (site v, first coordinate z in [0, len) where v is the minimiser, f(v)), entry k of lane t at
// stack[k * 256 + t] of the workgroup's region of (len + 2) * 256 entries: at most len + 2 sites,
// whatever len is.  v + 1 and z fit 16 bits each because the grids the entry points accept have no side
// above 46339.  A lane's steps are a chain of dependent memory accesses, so the column's values are
// loaded kDistAhead at a time before they are needed, and the walk back over the stack keeps the next
// four entries in registers.
constexpr int kDistAhead = 8;

__global__ __launch_bounds__(256) void dist_column_kernel(int *__restrict__ S, long long ncols, int len,
                                                          long long stride, int X, long long outer,
                                                          int border_empty, int2 *__restrict__ stack) {
    int2 *my = stack + (size_t)blockIdx.x * (size_t)(len + 2) * 256 + threadIdx.x;
    const long long ngroups = (2 * ncols + 255) / 256;
    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long lane = grp * 256 + threadIdx.x;
        if (lane >= 2 * ncols) continue;  // (no barrier below)
        const int sign = lane >= ncols ? 1 : 0;
        const long long c = lane - (sign ? ncols : 0);
        int *col = S + (size_t)(c / X) * (size_t)outer + (size_t)(c % X);
        int n = 0;                   // entries on the stack
        int tv = 0, tz = 0, tf = 0;  // the top entry
        auto site = [&](int q, int f) {
            while (n > 0) {  // the top loses its whole stretch to q: off
                // (a value below 2^31 plus a square of at most 46340^2: the sums fit 32 bits unsigned)
                const int dv = tz - tv, dq = tz - q;
                if ((unsigned)tf + (unsigned)(dv * dv) <= (unsigned)f + (unsigned)(dq * dq)) break;
                if (--n > 0) {
                    const int2 e = my[(size_t)(n - 1) * 256];
                    tv = (int)((unsigned)e.x & 0xffffu) - 1;
                    tz = (int)((unsigned)e.x >> 16);
                    tf = e.y;
                }
            }
            long long w = 0;  // first coordinate at which q is strictly better than the top
            if (n > 0) {
                const long long num =
                    (long long)((unsigned)f + (unsigned)(q * q)) - (long long)((unsigned)tf + (unsigned)(tv * tv));
                w = dist_floor_div(num, 2 * (q - tv)) + 1;
                if (w >= len) return;
            }
            tv = q;
            tz = (int)w;
            tf = f;
            my[(size_t)n * 256] = make_int2((int)((unsigned)(q + 1) | ((unsigned)w << 16)), f);
            ++n;
        };
        const bool border = sign == 0 && border_empty;
        const int none = sign == 0 ? kDistInf : -kDistInf;  // no site of the envelope's kind behind this value
        if (border) site(-1, 0);
        for (int j0 = 0; j0 < len; j0 += kDistAhead) {
            int s[kDistAhead];
#pragma unroll
            for (int u = 0; u < kDistAhead; ++u) s[u] = j0 + u < len ? col[(size_t)(j0 + u) * stride] : none;
#pragma unroll
            for (int u = 0; u < kDistAhead; ++u) {
                if (s[u] == none) continue;
                const int f = sign == 0 ? s[u] : -s[u];  // the partial distance at the other kind's voxels
                site(j0 + u, f > 0 ? f : 0);
            }
        }
        if (border) site(len, 0);
        // read the envelope back, front to end: the current entry, and the next four (z = len: none)
        auto entry = [&](int k) -> int2 { return k < n ? my[(size_t)k * 256] : make_int2((int)((unsigned)len << 16), 0); };
        int2 cur = entry(0), q0 = entry(1), q1 = entry(2), q2 = entry(3), q3 = entry(4);
        int k = 0;
        for (int j0 = 0; j0 < len; j0 += kDistAhead) {
            int s[kDistAhead];
#pragma unroll
            for (int u = 0; u < kDistAhead; ++u) s[u] = j0 + u < len ? col[(size_t)(j0 + u) * stride] : 0;
#pragma unroll
            for (int u = 0; u < kDistAhead; ++u) {
                const int j = j0 + u;
                if (j >= len) break;
                while ((int)((unsigned)q0.x >> 16) <= j) {
                    cur = q0;
                    q0 = q1;
                    q1 = q2;
                    q2 = q3;
                    q3 = entry(k + 5);
                    ++k;
                }
                if ((sign == 0) != (s[u] > 0)) continue;  // (the other kind's voxel)
                const int dj = j - ((int)((unsigned)cur.x & 0xffffu) - 1);
                const int val = n > 0 ? (int)((unsigned)cur.y + (unsigned)(dj * dj)) : kDistInf;  // (the least: it fits)
                col[(size_t)j * stride] = sign == 0 ? val : -val;
            }
        }
    }
}

// The field against the squared radius R -> bit plane.  A wave takes kDistWordsPerWave consecutive words,
// as in pass 1, a word per ballot.
//   grow = 0: in = (d > R), erosion of the set the field was built from
//   grow = 1: in = (d > 0 or -d <= R), its dilation
//   kind 0: out = in;  kind 1: out = orig & ~in (the voxels that leave `orig`);
//   kind 2: out = in & ~orig (those that join it).  Kinds 1 and 2 add their set bits to *count, one
//   add per workgroup.
__global__ __launch_bounds__(256) void dist_threshold_kernel(const int *__restrict__ S, const BitGrid g, int R,
                                                             int grow, int kind,
                                                             const unsigned long long *__restrict__ orig,
                                                             unsigned long long *__restrict__ out,
                                                             unsigned long long *__restrict__ count) {
    __shared__ unsigned s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    size_t wi = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kDistWordsPerWave;
    const int b = (int)(threadIdx.x & 63);
    unsigned mine = 0u;
    if (wi < nwords) {  // (the whole wave)
        int xw = (int)(wi % g.XW);
        size_t row = wi / g.XW;
        for (int k8 = 0; k8 < kDistWordsPerWave && wi < nwords; ++k8, ++wi) {
            const int x = 64 * xw + b;
            bool in = false;
            if (x < g.X) {
                const int s = S[row * (size_t)g.X + x];
                in = grow ? (s > 0 || -(long long)s <= (long long)R) : (s > R);
            }
            const unsigned long long m = __ballot(in);
            if (b == 0) {
                unsigned long long res = m;
                if (kind == 1) res = orig[wi] & ~m;
                if (kind == 2) res = m & ~orig[wi];
                out[wi] = res;
                if (kind) mine += (unsigned)__popcll(res);
            }
            if (++xw == g.XW) {
                xw = 0;
                ++row;
            }
        }
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(count, (unsigned long long)s_count);
}

}  // namespace arvx
