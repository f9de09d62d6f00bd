// The read ceiling of the pruned exact sweep's access pattern on MI355X: per 64-row tile a wave reads the first
// `c` of the row's 128-B stages (8 rows x 128 B per wave instruction, one stage in flight, as exact_kernel does) and then one
// `pitch`-byte line per row from a second buffer with lane = row (16 B per lane and instruction at a stride of `pitch`), all with
// non-temporal loads; the values go into a checksum so nothing is optimised away.  Prints TB/s of bytes REQUESTED.
//   prefix_stream [rows=10000000] [dim=768] [c=9] [pitch=192] [workgroups per CU=2] [lines as stages=0] [head=0] [pipelined=0] [seed rows=0] [keep=10]
//                 [survivors per 100000 rows=0] [survivor form=0]
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

// c = 0, lines as stages, one round ahead across rounds and tiles; surv != nullptr: after every `period` tiles of the wave, 64 survivors
__device__ __forceinline__ float pipe_body(const char* __restrict__ lines, uint64_t n_tiles, uint32_t pitch, int head, const v4f* __restrict__ hcode,
                                           const float* __restrict__ hrho, const float* __restrict__ hinv, const char* __restrict__ surv = nullptr,
                                           uint32_t period = 0, uint32_t row_bytes = 0, const float* __restrict__ sscale = nullptr,
                                           const unsigned char* __restrict__ sflag = nullptr) {
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t np = pitch >> 4;
    float acc = 0.f;
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
        }
        if (!more) break;
#pragma unroll
        for (int m = 0; m < 8; m++) cur[m] = nxt[m];
        if (last) { hs = hsn; hc = hcn; }
        t = t2; i = i2;
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
                                                   uint32_t row_bytes, const float* __restrict__ sscale, const unsigned char* __restrict__ sflag, float* out) {
    const float acc = pipe_body(lines, n_tiles, pitch, 2, hcode, hrho, hinv, surv, period, row_bytes, sscale, sflag);
    if (acc == 12345.678f) out[0] = acc;
}
// the seed's estimate pass: the pipelined pattern over the seed's tiles, then `keep` <= 64 whole rows of the wave's first tile
__global__ __launch_bounds__(256) void sweep_seed(const float* __restrict__ rows, const char* __restrict__ lines, uint64_t n_tiles, uint32_t ld, uint32_t pitch,
                                                  uint32_t keep, const v4f* __restrict__ hcode, const float* __restrict__ hrho, const float* __restrict__ hinv,
                                                  float* out) {
    float acc = pipe_body(lines, n_tiles, pitch, 2, hcode, hrho, hinv);
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lrow = lane >> 3, lslot = lane & 7;
    if (gw < n_tiles) {  // (its first tile is inside the seed: every row read is one of that tile's 64)
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
    for (int it = 0; it < 8; it++) {
        CK(hipEventRecord(a));
        if (surv) hipLaunchKernelGGL(sweep_gated, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, l, n_tiles, pitch, (const v4f*)hc, hr, hi, (const char*)d, period,
                                     sform ? ld : ld * 4, sform ? hr : (const float*)nullptr, (const unsigned char*)hc, o);
        else if (seed) hipLaunchKernelGGL(sweep_seed, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, d, l, seed / 64, ld, pitch, keep, (const v4f*)hc, hr, hi, o);
        else if (pipe) hipLaunchKernelGGL(sweep_pipe, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, l, n_tiles, pitch, head, (const v4f*)hc, hr, hi, o);
        else hipLaunchKernelGGL(sweep, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, d, l, n_tiles, ld, c, pitch, staged, head, (const v4f*)hc, hr, hi, o);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (it && ms < best) best = ms;
    }
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
