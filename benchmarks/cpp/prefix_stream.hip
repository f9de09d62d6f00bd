// The read ceiling of the pruned exact sweep's access pattern on MI355X: per 64-row tile a wave reads the first
// `c` of the row's 128-B stages (8 rows x 128 B per wave instruction, one stage in flight, as exact_kernel does) and then one
// `pitch`-byte line per row from a second buffer with lane = row (16 B per lane and instruction at a stride of `pitch`), all with
// non-temporal loads; the values go into a checksum so nothing is optimised away.  Prints TB/s of bytes REQUESTED.
//   prefix_stream [rows=10000000] [dim=768] [c=9] [pitch=192] [workgroups per CU=2] [lines as stages=0] [head=0] [pipelined=0] [seed rows=0] [keep=10]
//                 [survivors per 100000 rows=0] [survivor form=0] [few form=0] [few waves per 1000=0] [few rows=1]
//   (dim a multiple of 32, pitch of 16, <= 512; c = 0 reads no row stage)
// lines as stages = 1: the tile's 64 lines are read as the row stages are — eight 16-B pieces of every line per round, 8 lines x
// 128 B per wave instruction — which is how the four-bit form of the sweep fetches them
// head = 1: the tile's 64 inverse norms are read as well, one f32 per row with lane = row; head = 2: a 16-B record and two f32
// per row from three plain arrays, lane = row (the head of DESIGN.md 3.1b: stage 0's codes, rho_all and the inverse norm)
// pipelined = 1 (c = 0 and lines as stages only): the next round of lines, or the next tile's first round and its head, is asked
// for before the current round is summed, so a tile's first round does not wait behind the last tile's sums
// seed rows = N > 0 (c = 0, lines as stages, head = 2, pipelined): the pattern of the seed's estimate pass instead — the pipelined
// line / head pattern over the first N rows only, and then per wave `keep` WHOLE rows of its first tile, read as the sweep finishes
// queued rows: a 128-B stage of eight rows per wave instruction, the next stage in flight while one is summed
//   prefix_stream 10000000 768 0 384 2 1 2 1 312512 10
// survivors = S > 0 (c = 0, lines as stages, head = 2, pipelined, no seed): the gated launch's pattern with its survivors — S rows in
// 100 000 pass the gate (the headline's recorded rate: 1367), and whenever 64 of a wave's have gathered it reads them as the sweep
// finishes queued rows: rows scattered over the store, a 128-B stage of eight rows per wave instruction, the next stage in flight
// while one is summed.  survivor form = 0: their whole f32 rows (dim x 4 bytes, today's finish); 1: their int8 plane rows (dim bytes)
// and, lane = row, a 4-B scale and a 1-B flag each (the int8 check of DESIGN.md 3.1b: what all but a few survivors then cost)
//   prefix_stream 10000000 768 0 384 2 1 2 1 0 10 1367 0        prefix_stream 10000000 768 0 384 2 1 2 1 0 10 1367 1
// few form = F > 0 (arguments 13 to 15: form, waves per 1000 that have rows to finish, rows n <= 16): what the two launches do with a
// FEW whole f32 rows.  With survivors (form 1 of them): every wave ends with one more tile of plane rows behind its last tile (the end
// drain's dependent plane stages), and the chosen share of the waves then finishes n scattered f32 rows — there, and behind every
// mid-sweep tile of plane rows as well.  With seed rows: every wave finishes `keep` rows of its first tile (n = keep, every wave).
// F = 1: as the sweep's wide finish does — a 128-B stage of eight rows per wave instruction, rows past n re-reading the first, one
// stage in flight while one is summed: dim / 32 dependent round trips.  F = 2: as rounds — G = (n <= 8 ? 1 : 2) row groups, the eight
// instructions of a round ask for 8 / G stages of the n rows at once, the next round in flight while one is summed.  F = 4: the rows
// are not read at all.  F = 3: the three alternated five times in this process (1, 2, 4, 1, ..), every time and the means printed.
// F = 5 (with survivors): the few rows as rounds, and the end drain's tile of plane rows three ways, alternated five times: 32 queued
// rows as a dense tile (a stage per round trip, rows past 32 re-reading the first), as two stages per round, and not read.
//   prefix_stream 10000000 768 0 384 2 1 2 1 0 10 1367 1 3 330 1        prefix_stream 10000000 768 0 384 2 1 2 1 312512 10 0 0 3
//   hipcc -O3 --offload-arch=gfx950 prefix_stream.hip -o prefix_stream
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float v4f __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ __launch_bounds__(256) void sweep(const float* __restrict__ rows, const char* __restrict__ lines, uint64_t n_tiles, uint32_t ld,
                                             uint32_t c, uint32_t pitch, int staged, int head, const v4f* __restrict__ hcode, const float* __restrict__ hrho,
                                             const float* __restrict__ hinv, float* out) {
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t np = pitch >> 4;  // 16-B pieces of a line
    float acc = 0.f;
    for (uint64_t t = gw; t < n_tiles; t += nw) {
        const float* base = rows + t * 64 * (uint64_t)ld;
        if (head) acc += __builtin_nontemporal_load(hinv + t * 64 + lane);
        if (head > 1) {
            const v4f hc = __builtin_nontemporal_load(hcode + t * 64 + lane);
            acc += hc.x + hc.y + hc.z + hc.w + __builtin_nontemporal_load(hrho + t * 64 + lane);
        }
        for (uint32_t s = 0; s < c; s++) {  // s < c <= ld / 32: inside the row
            v4f r[8];
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load((const v4f*)(base + (uint64_t)(8 * m + lrow) * ld + s * 32 + lslot * 4));
#pragma unroll
            for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
        }
        if (staged) {
            for (uint32_t i = 0; i < np; i += 8) {
                const uint32_t pc = i + lslot < np ? i + lslot : np - 1;  // clamped to the line's last piece
                v4f r[8];
#pragma unroll
                for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load((const v4f*)(lines + (t * 64 + 8 * m + lrow) * (uint64_t)pitch + 16 * pc));
#pragma unroll
                for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
            }
            continue;
        }
        const v4f* lp = (const v4f*)(lines + (t * 64 + lane) * (uint64_t)pitch);
        for (uint32_t i = 0; i < np; i += 8) {
            v4f r[8];
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load(lp + (i + m < np ? i + m : np - 1));  // clamped to the line's last piece
#pragma unroll
            for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
        }
    }
    if (acc == 12345.678f) out[0] = acc;
}

// 64 survivors of a wave, scattered over the store (every row index below n_rows): row_bytes each (whole 128-B stages), as the sweep
// finishes queued rows; sscale != nullptr: a scale and a flag per row as well, lane = row
__device__ __forceinline__ float finish64(const char* __restrict__ surv, uint64_t n_rows, uint32_t row_bytes, uint64_t t, const float* __restrict__ sscale,
                                          const unsigned char* __restrict__ sflag) {
    const int lane = threadIdx.x & 63;
    const int lrow = lane >> 3, lslot = lane & 7;
    float acc = 0.f;
    auto row_of = [&](uint32_t i) { return ((t * 64 + i) * 0x9E3779B97F4A7C15ull >> 20) % n_rows; };
    if (sscale) acc += __builtin_nontemporal_load(sscale + row_of(lane)) + (float)__builtin_nontemporal_load(sflag + row_of(lane));
    const char* rp[8];
#pragma unroll
    for (int m = 0; m < 8; m++) rp[m] = surv + row_of(8 * m + lrow) * row_bytes + lslot * 16;
    v4f r[8], rn[8];
#pragma unroll
    for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load((const v4f*)rp[m]);
    for (uint32_t s = 0; s < row_bytes / 128; s++) {
        if (s + 1 < row_bytes / 128) {
#pragma unroll
            for (int m = 0; m < 8; m++) rn[m] = __builtin_nontemporal_load((const v4f*)(rp[m] + (s + 1) * 128));
        }
#pragma unroll
        for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
#pragma unroll
        for (int m = 0; m < 8; m++) r[m] = rn[m];
    }
    return acc;
}

// n <= 16 whole rows of row_bytes (whole 128-B stages), rows pick(0 .. n - 1); form 1: as finish64 reads 64 (rows past n re-read the
// first), form 2: as rounds of 8 / G stages of G = (n <= 8 ? 1 : 2) row groups, a stage past the last clamped to it
struct Few {
    int form;        // 0 / 4: nothing is read
    uint32_t share;  // waves per 1000 that have rows
    uint32_t n;
    int edrain;      // the end drain's tile of plane rows: 0 = a dense tile of 64, 1 / 2 = 32 queued rows as one / two stages per round, 3 = not read
};
// the end drain's plane rows when n <= 32 wait: rows past n re-read the first (as the sweep's finishes do); two = 0: a stage of the
// 64-row tile per round trip, two = 1: the eight instructions ask for TWO stages of the 32 rows (a stage past the last clamped)
__device__ __forceinline__ float finish_plane32(const char* __restrict__ surv, uint64_t n_rows, uint32_t row_bytes, uint64_t t, uint32_t n, int two,
                                                const float* __restrict__ sscale, const unsigned char* __restrict__ sflag) {
    const int lane = threadIdx.x & 63;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t nst = row_bytes / 128, S = two ? 2u : 1u;
    float acc = 0.f;
    auto row_of = [&](uint32_t i) { return ((t * 64 + (i < n ? i : 0u)) * 0x9E3779B97F4A7C15ull >> 20) % n_rows; };
    if (sscale) acc += __builtin_nontemporal_load(sscale + row_of(lane)) + (float)__builtin_nontemporal_load(sflag + row_of(lane));
    const char* rp[8];
#pragma unroll
    for (int m = 0; m < 8; m++) rp[m] = surv + row_of(8 * (two ? m & 3 : m) + lrow) * row_bytes + lslot * 16;
    v4f r[8], rn[8];
    auto load_round = [&](v4f* d, uint32_t s0) {
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t s = s0 + (two ? (uint32_t)m >> 2 : 0u), sc = s < nst ? s : nst - 1;
            d[m] = __builtin_nontemporal_load((const v4f*)(rp[m] + sc * 128));
        }
    };
    load_round(r, 0);
    for (uint32_t s0 = 0; s0 < nst; s0 += S) {
        if (s0 + S < nst) load_round(rn, s0 + S);
#pragma unroll
        for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
#pragma unroll
        for (int m = 0; m < 8; m++) r[m] = rn[m];
    }
    return acc;
}
template <class Pick>
__device__ __forceinline__ float finish_few(const char* __restrict__ base, uint32_t row_bytes, uint32_t n, int form, Pick pick) {
    const int lane = threadIdx.x & 63;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t nst = row_bytes / 128;
    float acc = 0.f;
    v4f r[8], rn[8];
    if (form == 1) {
        const char* rp[8];
#pragma unroll
        for (int m = 0; m < 8; m++) rp[m] = base + pick(8 * m + lrow < n ? 8 * m + lrow : 0u) * row_bytes + lslot * 16;
#pragma unroll
        for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load((const v4f*)rp[m]);
        for (uint32_t s = 0; s < nst; s++) {
            if (s + 1 < nst) {
#pragma unroll
                for (int m = 0; m < 8; m++) rn[m] = __builtin_nontemporal_load((const v4f*)(rp[m] + (s + 1) * 128));
            }
#pragma unroll
            for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = rn[m];
        }
    } else if (form == 2) {
        const uint32_t gsh = n <= 8 ? 0u : 1u, S = 8u >> gsh;
        const char* rp0 = base + pick((uint32_t)lrow < n ? (uint32_t)lrow : 0u) * row_bytes + lslot * 16;
        const char* rp1 = base + pick(8u + lrow < n ? 8u + lrow : 0u) * row_bytes + lslot * 16;
        auto load_round = [&](v4f* d, uint32_t s0) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t s = s0 + ((uint32_t)m >> gsh), sc = s < nst ? s : nst - 1;
                d[m] = __builtin_nontemporal_load((const v4f*)((((uint32_t)m & ((1u << gsh) - 1u)) ? rp1 : rp0) + sc * 128));
            }
        };
        load_round(r, 0);
        for (uint32_t s0 = 0; s0 < nst; s0 += S) {
            if (s0 + S < nst) load_round(rn, s0 + S);
#pragma unroll
            for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = rn[m];
        }
    }
    return acc;
}
__device__ __forceinline__ bool few_chosen(uint32_t gw, uint64_t salt, uint32_t share) {
    return (((gw + 1) * 0x9E3779B97F4A7C15ull + salt * 0xD1B54A32D192ED03ull) >> 33) % 1000u < share;
}

// c = 0, lines as stages, one round ahead across rounds and tiles; surv != nullptr: after every `period` tiles of the wave, 64 survivors
__device__ __forceinline__ float pipe_body(const char* __restrict__ lines, uint64_t n_tiles, uint32_t pitch, int head, const v4f* __restrict__ hcode,
                                           const float* __restrict__ hrho, const float* __restrict__ hinv, const char* __restrict__ surv = nullptr,
                                           uint32_t period = 0, uint32_t row_bytes = 0, const float* __restrict__ sscale = nullptr,
                                           const unsigned char* __restrict__ sflag = nullptr, const char* __restrict__ frows = nullptr,
                                           uint32_t frow_bytes = 0, Few few = Few{0, 0, 0, 0}) {
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t np = pitch >> 4;
    float acc = 0.f;
    // a tile of plane rows, and behind it on the chosen waves the few f32 rows (few.form != 0 only)
    auto drain_few = [&](uint64_t salt) {
        const uint64_t n_rows = n_tiles * 64;
        if (few_chosen(gw, salt, few.share))
            acc += finish_few(frows, frow_bytes, few.n, few.form, [&](uint32_t i) { return ((salt * 64 + 17 + i) * 0x9E3779B97F4A7C15ull >> 20) % n_rows; });
    };
    v4f cur[8], nxt[8], hc = {0.f, 0.f, 0.f, 0.f}, hcn = {0.f, 0.f, 0.f, 0.f};
    float hs = 0.f, hsn = 0.f;
    uint64_t t = gw;
    uint32_t i = 0, tiles_done = 0;
    if (t >= n_tiles) return acc;
#pragma unroll
    for (int m = 0; m < 8; m++) cur[m] = __builtin_nontemporal_load((const v4f*)(lines + (t * 64 + 8 * m + lrow) * (uint64_t)pitch + 16 * (lslot < np ? lslot : np - 1)));
    if (head) hs = __builtin_nontemporal_load(hinv + t * 64 + lane);
    if (head > 1) { hc = __builtin_nontemporal_load(hcode + t * 64 + lane); hs += __builtin_nontemporal_load(hrho + t * 64 + lane); }
    for (;;) {
        const bool last = i + 8 >= np;
        const uint64_t t2 = last ? t + nw : t;
        const uint32_t i2 = last ? 0 : i + 8;
        const bool more = t2 < n_tiles;  // t2 < n_tiles: inside the arrays
        if (more) {
            const uint32_t pc = i2 + lslot < np ? i2 + lslot : np - 1;
#pragma unroll
            for (int m = 0; m < 8; m++) nxt[m] = __builtin_nontemporal_load((const v4f*)(lines + (t2 * 64 + 8 * m + lrow) * (uint64_t)pitch + 16 * pc));
            if (last && head) hsn = __builtin_nontemporal_load(hinv + t2 * 64 + lane);
            if (last && head > 1) { hcn = __builtin_nontemporal_load(hcode + t2 * 64 + lane); hsn += __builtin_nontemporal_load(hrho + t2 * 64 + lane); }
        }
#pragma unroll
        for (int m = 0; m < 8; m++) acc += cur[m].x + cur[m].y + cur[m].z + cur[m].w;
        if (i == 0) acc += hs + hc.x + hc.y + hc.z + hc.w;
        if (surv && last && ++tiles_done == period) {
            tiles_done = 0;
            acc += finish64(surv, n_tiles * 64, row_bytes, t, sscale, sflag);
            if (few.form) drain_few(t);
        }
        if (!more) break;
#pragma unroll
        for (int m = 0; m < 8; m++) cur[m] = nxt[m];
        if (last) { hs = hsn; hc = hcn; }
        t = t2; i = i2;
    }
    if (few.form) {  // the end of the sweep: what is left in the queue as one more tile of plane rows, then the few
        if (few.edrain == 0) acc += finish64(surv, n_tiles * 64, row_bytes, n_tiles + gw, sscale, sflag);
        else if (few.edrain < 3) acc += finish_plane32(surv, n_tiles * 64, row_bytes, n_tiles + gw, 32, few.edrain == 2, sscale, sflag);
        drain_few(n_tiles + gw);
    }
    return acc;
}
__global__ __launch_bounds__(256) void sweep_pipe(const char* __restrict__ lines, uint64_t n_tiles, uint32_t pitch, int head, const v4f* __restrict__ hcode,
                                                  const float* __restrict__ hrho, const float* __restrict__ hinv, float* out) {
    const float acc = pipe_body(lines, n_tiles, pitch, head, hcode, hrho, hinv);
    if (acc == 12345.678f) out[0] = acc;
}
// the gated launch with its survivors
__global__ __launch_bounds__(256) void sweep_gated(const char* __restrict__ lines, uint64_t n_tiles, uint32_t pitch, const v4f* __restrict__ hcode,
                                                   const float* __restrict__ hrho, const float* __restrict__ hinv, const char* __restrict__ surv, uint32_t period,
                                                   uint32_t row_bytes, const float* __restrict__ sscale, const unsigned char* __restrict__ sflag,
                                                   const char* __restrict__ frows, uint32_t frow_bytes, Few few, float* out) {
    const float acc = pipe_body(lines, n_tiles, pitch, 2, hcode, hrho, hinv, surv, period, row_bytes, sscale, sflag, frows, frow_bytes, few);
    if (acc == 12345.678f) out[0] = acc;
}
// the seed's estimate pass: the pipelined pattern over the seed's tiles, then `keep` <= 64 whole rows of the wave's first tile
__global__ __launch_bounds__(256) void sweep_seed(const float* __restrict__ rows, const char* __restrict__ lines, uint64_t n_tiles, uint32_t ld, uint32_t pitch,
                                                  uint32_t keep, const v4f* __restrict__ hcode, const float* __restrict__ hrho, const float* __restrict__ hinv,
                                                  int fform, float* out) {
    float acc = pipe_body(lines, n_tiles, pitch, 2, hcode, hrho, hinv);
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lrow = lane >> 3, lslot = lane & 7;
    if (fform && gw < n_tiles) {  // (few form: the same rows of the wave's first tile, keep <= 16)
        acc += finish_few((const char*)(rows + (uint64_t)gw * 64 * ld), ld * 4, keep, fform, [&](uint32_t i) { return (uint64_t)((i * 5) & 63); });
    } else if (gw < n_tiles) {  // (its first tile is inside the seed: every row read is one of that tile's 64)
        const float* rp[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t i = 8 * m + lrow;
            rp[m] = rows + ((uint64_t)gw * 64 + (i < keep ? (i * 5) & 63 : 0)) * ld + lslot * 4;  // (past keep: the first row again, as the sweep does)
        }
        v4f r[8], rn[8];
#pragma unroll
        for (int m = 0; m < 8; m++) r[m] = __builtin_nontemporal_load((const v4f*)rp[m]);
        for (uint32_t s = 0; s < ld / 32; s++) {
            if (s + 1 < ld / 32) {
#pragma unroll
                for (int m = 0; m < 8; m++) rn[m] = __builtin_nontemporal_load((const v4f*)(rp[m] + (s + 1) * 32));
            }
#pragma unroll
            for (int m = 0; m < 8; m++) acc += r[m].x + r[m].y + r[m].z + r[m].w;
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = rn[m];
        }
    }
    if (acc == 12345.678f) out[0] = acc;
}

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    const uint32_t ld = argc > 2 ? (uint32_t)atoi(argv[2]) : 768u;
    const uint32_t c = argc > 3 ? (uint32_t)atoi(argv[3]) : 9u;
    const uint32_t pitch = argc > 4 ? (uint32_t)atoi(argv[4]) : 192u;
    const int per_cu = argc > 5 ? atoi(argv[5]) : 2;
    const int staged = argc > 6 ? atoi(argv[6]) : 0;
    const int head = argc > 7 ? atoi(argv[7]) : 0;
    const int pipe = argc > 8 ? atoi(argv[8]) : 0;
    const uint64_t seed = argc > 9 ? strtoull(argv[9], nullptr, 10) : 0ull;
    const uint32_t keep = argc > 10 ? (uint32_t)atoi(argv[10]) : 10u;
    const uint32_t surv = argc > 11 ? (uint32_t)atoi(argv[11]) : 0u;
    const int sform = argc > 12 ? atoi(argv[12]) : 0;
    const int fform = argc > 13 ? atoi(argv[13]) : 0;
    const uint32_t fshare = argc > 14 ? (uint32_t)atoi(argv[14]) : 0u;
    const uint32_t fn = argc > 15 ? (uint32_t)atoi(argv[15]) : 1u;
    if (fform && (fform < 1 || fform > 5 || (fform == 5 && !surv) || !(surv ? sform == 1 : seed != 0) || fshare > 1000 || fn < 1 || fn > 16 || (seed && keep > 16) || ld % 32)) {
        printf("bad arguments\n");
        return 1;
    }
    if (surv && (seed || !pipe || head != 2 || surv > 50000 || sform < 0 || sform > 1 || ld % 128)) {
        printf("bad arguments\n");
        return 1;
    }
    const uint32_t period = surv ? (100000u + surv / 2) / surv : 0u;  // tiles of a wave between two finishes of 64 survivors
    if (seed && (seed < 64 || seed > n || !pipe || head != 2 || keep < 1 || keep > 64)) {
        printf("bad arguments\n");
        return 1;
    }
    if (head < 0 || head > 2 || pipe < 0 || pipe > 1 || (pipe && (c || !staged))) {
        printf("bad arguments\n");
        return 1;
    }
    if (n < 64 || ld == 0 || ld % 32 || c > ld / 32 || pitch < 16 || pitch % 16 || pitch > 512 || per_cu < 1 || per_cu > 8) {
        printf("bad arguments\n");
        return 1;
    }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const uint64_t n_tiles = n / 64;  // whole tiles only
    float *d, *o, *hr, *hi;
    char *l, *hc;
    CK(hipMalloc(&hc, n_tiles * 64 * 16)); CK(hipMalloc(&hr, n_tiles * 64 * 4)); CK(hipMalloc(&hi, n_tiles * 64 * 4));
    CK(hipMemset(hc, 0, n_tiles * 64 * 16)); CK(hipMemset(hr, 0, n_tiles * 64 * 4)); CK(hipMemset(hi, 0, n_tiles * 64 * 4));
    CK(hipMalloc(&d, n_tiles * 64 * (size_t)ld * 4)); CK(hipMalloc(&l, n_tiles * 64 * (size_t)pitch)); CK(hipMalloc(&o, 4));
    CK(hipMemset(d, 0, n_tiles * 64 * (size_t)ld * 4)); CK(hipMemset(l, 0, n_tiles * 64 * (size_t)pitch));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e9f;
    int edrain_now = 0;
    int form_now = fform == 3 ? 1 : fform == 5 ? 2 : fform;  // (4: the few rows are not read; the kernels take that as a form that reads nothing)
    auto timed = [&]() {
      best = 1e9f;
      for (int it = 0; it < 8; it++) {
        CK(hipEventRecord(a));
        if (surv) hipLaunchKernelGGL(sweep_gated, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, l, n_tiles, pitch, (const v4f*)hc, hr, hi, (const char*)d, period,
                                     sform ? ld : ld * 4, sform ? hr : (const float*)nullptr, (const unsigned char*)hc, (const char*)d, ld * 4, Few{form_now, fshare, fn, edrain_now}, o);
        else if (seed) hipLaunchKernelGGL(sweep_seed, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, d, l, seed / 64, ld, pitch, keep, (const v4f*)hc, hr, hi,
                                          form_now, o);
        else if (pipe) hipLaunchKernelGGL(sweep_pipe, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, l, n_tiles, pitch, head, (const v4f*)hc, hr, hi, o);
        else hipLaunchKernelGGL(sweep, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, d, l, n_tiles, ld, c, pitch, staged, head, (const v4f*)hc, hr, hi, o);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (it && ms < best) best = ms;
      }
    };
    if (fform == 3) {  // the three forms alternated in this process
        const int forms[3] = {1, 2, 4};
        const char* names[3] = {"dim / 32 dependent stages", "rounds of several stages", "not read"};
        double sum[3] = {0, 0, 0};
        printf("%s, the few rows (%u per finish%s) as:\n", surv ? "gated launch" : "estimate pass", surv ? fn : keep, surv ? "" : ", every wave");
        if (surv) printf("  (%u waves in 1000 finish them behind every tile of plane rows, the end drain's included)\n", fshare);
        for (int rnd = 0; rnd < 5; rnd++)
            for (int f = 0; f < 3; f++) {
                form_now = forms[f];
                timed();
                sum[f] += best;
                printf("  run %d  %-28s %.4f ms\n", rnd + 1, names[f], best);
            }
        for (int f = 0; f < 3; f++) printf("  mean   %-28s %.4f ms\n", names[f], sum[f] / 5);
        printf("  dependent stages minus rounds: %.1f us; dependent stages minus not read: %.1f us\n", (sum[0] - sum[1]) / 5 * 1e3, (sum[0] - sum[2]) / 5 * 1e3);
        return 0;
    }
    if (fform == 5) {  // the end drain's plane rows, the few f32 rows read as rounds: 32 queued rows as one and as two stages per round, and not at all
        const int forms[3] = {1, 2, 3};
        const char* names[3] = {"32 rows, a stage per round", "32 rows, two stages per round", "not read"};
        double sum[3] = {0, 0, 0};
        printf("gated launch, the end drain's plane rows as (the few f32 rows, %u per finish on %u waves in 1000, as rounds):\n", fn, fshare);
        for (int rnd = 0; rnd < 5; rnd++)
            for (int f = 0; f < 3; f++) {
                edrain_now = forms[f];
                timed();
                sum[f] += best;
                printf("  run %d  %-30s %.4f ms\n", rnd + 1, names[f], best);
            }
        for (int f = 0; f < 3; f++) printf("  mean   %-30s %.4f ms\n", names[f], sum[f] / 5);
        printf("  one stage minus two stages per round: %.1f us; one stage per round minus not read: %.1f us\n", (sum[0] - sum[1]) / 5 * 1e3, (sum[0] - sum[2]) / 5 * 1e3);
        return 0;
    }
    timed();
    if (seed) {
        const uint64_t waves = (uint64_t)prop.multiProcessorCount * per_cu * 4, with_rows = waves < seed / 64 ? waves : seed / 64;
        const double sb = (double)(seed / 64) * 64 * (pitch + 24.0) + (double)with_rows * keep * ld * 4.0;
        printf("estimate pass: %llu of %llu rows, dim %u, pitch %u, head 24 B, pipelined, %u whole rows on each of %llu waves, %d workgroups per CU: %.4f ms  %.3f GB requested  %.2f TB/s\n",
               (unsigned long long)(seed / 64 * 64), (unsigned long long)n, ld, pitch, keep, (unsigned long long)with_rows, per_cu, best, sb / 1e9, sb / best / 1e9);
        return 0;
    }
    if (surv) {
        const uint64_t waves = (uint64_t)prop.multiProcessorCount * per_cu * 4;
        uint64_t finishes = 0;  // wave w owns tiles w, w + waves, ...: one finish per `period` of them
        for (uint64_t w = 0; w < waves && w < n_tiles; w++) finishes += ((n_tiles - w + waves - 1) / waves) / period;
        const double per_row = sform ? ld + 5.0 : ld * 4.0;
        const double gb = (double)n_tiles * 64 * (pitch + 24.0) + (double)finishes * 64 * per_row;
        printf("gated launch: rows %llu dim %u pitch %u head 24 B pipelined, %llu survivors (%u in 100000) read as %s, %d workgroups per CU: %.4f ms  %.3f GB requested  %.2f TB/s\n",
               (unsigned long long)n, ld, pitch, (unsigned long long)(finishes * 64), surv, sform ? "int8 plane rows + scale + flag" : "f32 rows", per_cu, best, gb / 1e9,
               gb / best / 1e9);
        return 0;
    }
    const double bytes = (double)n_tiles * 64 * (c * 128.0 + pitch + (head == 2 ? 24 : head ? 4 : 0));
    printf("rows %llu dim %u c %u pitch %u%s%s%s, %d workgroups per CU: %.3f ms  %.3f GB requested  %.2f TB/s\n", (unsigned long long)n, ld, c, pitch, staged ? " (lines as stages)" : "",
           head == 2 ? " head 24 B" : head ? " inverse norms" : "", pipe ? " pipelined" : "", per_cu,
           best, bytes / 1e9, bytes / best / 1e9);
    return 0;
}
