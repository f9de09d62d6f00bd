// The read ceiling of the pruned exact sweep's access pattern on MI355X: per 64-row tile a wave reads the first
// `c` of the row's 128-B stages (8 rows x 128 B per wave instruction, one stage in flight, as exact_kernel does) and then one
// `pitch`-byte line per row from a second buffer with lane = row (16 B per lane and instruction at a stride of `pitch`), all with
// non-temporal loads; the values go into a checksum so nothing is optimised away.  Prints TB/s of bytes REQUESTED.
//   prefix_stream [rows=10000000] [dim=768] [c=9] [pitch=192] [workgroups per CU=2] [lines as stages=0]
//   (dim a multiple of 32, pitch of 16, <= 512)
// lines as stages = 1: the tile's 64 lines are read as the row stages are — eight 16-B pieces of every line per round, 8 lines x
// 128 B per wave instruction — which is how the four-bit form of the sweep fetches them
//   hipcc -O3 --offload-arch=gfx950 prefix_stream.hip -o prefix_stream
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float v4f __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ __launch_bounds__(256) void sweep(const float* __restrict__ rows, const char* __restrict__ lines, uint64_t n_tiles, uint32_t ld,
                                             uint32_t c, uint32_t pitch, int staged, float* out) {
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    const uint32_t np = pitch >> 4;  // 16-B pieces of a line
    float acc = 0.f;
    for (uint64_t t = gw; t < n_tiles; t += nw) {
        const float* base = rows + t * 64 * (uint64_t)ld;
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

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    const uint32_t ld = argc > 2 ? (uint32_t)atoi(argv[2]) : 768u;
    const uint32_t c = argc > 3 ? (uint32_t)atoi(argv[3]) : 9u;
    const uint32_t pitch = argc > 4 ? (uint32_t)atoi(argv[4]) : 192u;
    const int per_cu = argc > 5 ? atoi(argv[5]) : 2;
    const int staged = argc > 6 ? atoi(argv[6]) : 0;
    if (n < 64 || ld == 0 || ld % 32 || c < 1 || c > ld / 32 || pitch < 16 || pitch % 16 || pitch > 512 || per_cu < 1 || per_cu > 8) {
        printf("bad arguments\n");
        return 1;
    }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const uint64_t n_tiles = n / 64;  // whole tiles only
    float *d, *o;
    char* l;
    CK(hipMalloc(&d, n_tiles * 64 * (size_t)ld * 4)); CK(hipMalloc(&l, n_tiles * 64 * (size_t)pitch)); CK(hipMalloc(&o, 4));
    CK(hipMemset(d, 0, n_tiles * 64 * (size_t)ld * 4)); CK(hipMemset(l, 0, n_tiles * 64 * (size_t)pitch));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e9f;
    for (int it = 0; it < 8; it++) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(sweep, dim3(prop.multiProcessorCount * per_cu), dim3(256), 0, 0, d, l, n_tiles, ld, c, pitch, staged, o);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (it && ms < best) best = ms;
    }
    const double bytes = (double)n_tiles * 64 * (c * 128.0 + pitch);
    printf("rows %llu dim %u c %u pitch %u%s, %d workgroups per CU: %.3f ms  %.3f GB requested  %.2f TB/s\n", (unsigned long long)n, ld, c, pitch, staged ? " (lines as stages)" : "", per_cu,
           best, bytes / 1e9, bytes / best / 1e9);
    return 0;
}
