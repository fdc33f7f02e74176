// Standalone microbench: what the ring-write shapes of the broadcast fan-out
// reach on the bench's 10,000 x 1 MiB ring layout, 2.87 GB per launch
// (256 records of 1,120 B per user).  Companion of k3_roofline.hip, same
// warm-up and 10 timed launches per variant:
//   (a) k3_roofline.hip's k3_writeonly: unit-per-lane flat index, two 64-bit
//       divisions per 16 B unit, NT stores
//   (b) (a) with 32-bit magic divisions
//   (c) the dense-run shape: a 256-thread workgroup holds a chunk of a
//       32-record image in registers (constants) and stores it to G users in
//       turn; swept over store flavour, G, chunking and grid mapping
//   (d) (c) with the registers loaded from a 287 KB device image first
//
//   hipcc -O3 --offload-arch=gfx950 scripts/k3_write_shapes.hip -o a.out && ./a.out
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

#include "../csrc/common/divmagic.h"
#include "../csrc/hip/dataplane.h"

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

template <int NT>
__device__ __forceinline__ void st16(void* dst, v4u v) {
    if (NT) __builtin_nontemporal_store(v, (v4u*)dst);
    else *(v4u*)dst = v;
}

__global__ void __launch_bounds__(256) k3_writeonly(
    int64_t n_pairs, int32_t units, int64_t ring_bytes, int32_t n_msgs,
    uint64_t rec, uint8_t* egress)
{
    const int64_t n_units = n_pairs * units;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    v4u v = {1u, 2u, 3u, 4u};
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_units; f += stride) {
        const int64_t p = f / units;
        const int32_t unit = (int32_t)(f - p * units);
        const int64_t u = p / n_msgs;
        const int64_t m = p - u * n_msgs;
        uint8_t* dst = egress + u * ring_bytes + m * rec + (size_t)unit * 16;
        __builtin_nontemporal_store(v, (v4u*)dst);
    }
}

__global__ void __launch_bounds__(256) k3_writeonly_magic(
    int64_t n_pairs, int32_t units, uint32_t um, int32_t ush, int64_t ring_bytes,
    int32_t n_msgs, uint32_t mm, int32_t msh, uint64_t rec, uint8_t* egress)
{
    const int64_t n_units = n_pairs * units;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    v4u v = {1u, 2u, 3u, 4u};
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_units; f += stride) {
        const uint32_t f32 = (uint32_t)f;      // 2.56 M pairs x 70 units < 2^31
        const uint32_t p = (uint32_t)(((uint64_t)f32 * um) >> ush);
        const uint32_t unit = f32 - p * (uint32_t)units;
        const uint32_t u = (uint32_t)(((uint64_t)p * mm) >> msh);
        const uint32_t m = p - u * (uint32_t)n_msgs;
        uint8_t* dst = egress + (int64_t)u * ring_bytes + (uint64_t)m * rec + (size_t)unit * 16;
        __builtin_nontemporal_store(v, (v4u*)dst);
    }
}

// The dense-run shape.  V dword4 registers per thread hold units
// [c * chunk_units, + chunk_units) of block b's image; MAP 0 orders the
// workgroups (block, user group, chunk), MAP 1 (user group, block, chunk).
template <int NT, int V, bool LOAD, int MAP>
__global__ void __launch_bounds__(256) dense_run(
    const v4u* __restrict__ image, int32_t image_units, int32_t n_chunks, int32_t chunk_units,
    int32_t n_users, int32_t group, int64_t ring_bytes, uint64_t rec, uint8_t* egress)
{
    int b, g, c;
    if (MAP == 0) {
        b = blockIdx.y; g = blockIdx.x / n_chunks; c = blockIdx.x - g * n_chunks;
    } else {
        g = blockIdx.y; b = blockIdx.x / n_chunks; c = blockIdx.x - b * n_chunks;
    }
    const int lo = c * chunk_units + (int)threadIdx.x;
    const int hi = min(image_units, (c + 1) * chunk_units);
    v4u v[V];
    #pragma unroll
    for (int k = 0; k < V; ++k) {
        const int unit = lo + k * 256;
        v[k] = v4u{1u, 2u, 3u, (uint32_t)k};
        if (LOAD && unit < hi) v[k] = image[(size_t)b * image_units + unit];
    }
    if (lo >= hi) return;
    const int u1 = min(n_users, (g + 1) * group);
    for (int u = g * group; u < u1; ++u) {
        uint8_t* dst = egress + (int64_t)u * ring_bytes + (uint64_t)b * 32 * rec + (size_t)lo * 16;
        #pragma unroll
        for (int k = 0; k < V; ++k)
            if (lo + k * 256 < hi) st16<NT>(dst + (size_t)k * 4096, v[k]);
    }
}

static hipEvent_t ev_a, ev_b;

template <typename F>
static float time_us(F launch) {
    for (int i = 0; i < 3; i++) launch();
    (void)hipEventRecord(ev_a);
    for (int i = 0; i < 10; i++) launch();
    (void)hipEventRecord(ev_b); (void)hipEventSynchronize(ev_b);
    float ms; (void)hipEventElapsedTime(&ms, ev_a, ev_b);
    return ms * 100.0f;
}

struct DenseCfg { int nt, nch, load, map, group; };

template <int NT, int V, bool LOAD, int MAP>
static float run_dense(const DenseCfg& cfg, const v4u* image, int32_t image_units,
                       int32_t n_chunks, int32_t chunk_units, int32_t n_users,
                       int64_t ring_bytes, uint64_t rec, int32_t n_blocks, uint8_t* egress) {
    const uint32_t gx = (uint32_t)dense_grid_x(n_users, cfg.group, 1);
    const dim3 grid = MAP == 0 ? dim3(gx * n_chunks, n_blocks) : dim3(n_blocks * n_chunks, gx);
    return time_us([&] {
        hipLaunchKernelGGL((dense_run<NT, V, LOAD, MAP>), grid, dim3(256), 0, 0, image,
                           image_units, n_chunks, chunk_units, n_users, cfg.group, ring_bytes,
                           rec, egress);
    });
}

template <int V>
static float dispatch_dense(const DenseCfg& c, const v4u* image, int32_t iu, int32_t nch,
                            int32_t cu, int32_t nu, int64_t rb, uint64_t rec, int32_t nb,
                            uint8_t* eg) {
#define RD(NT, LOAD, MAP) run_dense<NT, V, LOAD, MAP>(c, image, iu, nch, cu, nu, rb, rec, nb, eg)
    if (c.nt) {
        if (c.load) return c.map ? RD(1, true, 1) : RD(1, true, 0);
        return c.map ? RD(1, false, 1) : RD(1, false, 0);
    }
    if (c.load) return c.map ? RD(0, true, 1) : RD(0, true, 0);
    return c.map ? RD(0, false, 1) : RD(0, false, 0);
#undef RD
}

int main() {
    const int64_t n_users = 10000, n_msgs = 256;
    const uint64_t rec = 1120;       // ring_rec(1104) for the 1 KiB bench
    const int32_t units = rec / 16;
    const int64_t ring_bytes = 1 << 20;
    const int64_t n_pairs = n_users * n_msgs;
    const int32_t n_blocks = n_msgs / 32, image_units = units * 32;
    uint8_t* egress;
    if (hipMalloc(&egress, n_users * ring_bytes) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    v4u* image;
    if (hipMalloc(&image, n_msgs * rec) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    (void)hipMemset(image, 0x5a, n_msgs * rec);
    const int64_t bytes = n_pairs * (int64_t)rec;
    (void)hipEventCreate(&ev_a); (void)hipEventCreate(&ev_b);
    auto tbs = [&](float us) { return bytes / (us * 1e-6) / 1e12; };

    float us = time_us([&] {
        hipLaunchKernelGGL(k3_writeonly, dim3(16384), dim3(256), 0, 0, n_pairs, units,
                           ring_bytes, (int32_t)n_msgs, rec, egress);
    });
    printf("(a) flat, 64-bit div, nt:        %6.0f us  %.2f TB/s\n", us, tbs(us));
    uint32_t um, mm; int32_t ush, msh;
    u32_div_magic(units, &um, &ush);
    u32_div_magic((int32_t)n_msgs, &mm, &msh);
    us = time_us([&] {
        hipLaunchKernelGGL(k3_writeonly_magic, dim3(16384), dim3(256), 0, 0, n_pairs, units, um,
                           ush, ring_bytes, (int32_t)n_msgs, mm, msh, rec, egress);
    });
    printf("(b) flat, magic div, nt:         %6.0f us  %.2f TB/s\n", us, tbs(us));

    // chunkings: the whole 35,840 B image in one workgroup (9 registers per
    // thread), or dense_geom's split (2 chunks of 1,152 units, 5 registers)
    const DenseGeom geo = dense_geom(units);
    for (int load = 0; load < 2; ++load) {
        const int reps = load ? 3 : 1;   // (d) repeated: its spread decides
        for (int rep = 0; rep < reps; ++rep)
            for (int nch : {1, geo.n_chunks})
                for (int nt = 1; nt >= 0; --nt)
                    for (int map = 0; map < 2; ++map)
                        for (int group : {8, 16, 32, 64}) {
                            DenseCfg c{nt, nch, load, map, group};
                            const int32_t cu = nch == 1 ? image_units : geo.chunk_units;
                            us = nch == 1
                                ? dispatch_dense<9>(c, image, image_units, 1, cu, (int32_t)n_users,
                                                    ring_bytes, rec, n_blocks, egress)
                                : dispatch_dense<DENSE_MAX_V>(c, image, image_units, nch, cu,
                                                              (int32_t)n_users, ring_bytes, rec,
                                                              n_blocks, egress);
                            printf("(%c) dense chunks=%d %s map=%d G=%2d%s: %6.0f us  %.2f TB/s\n",
                                   load ? 'd' : 'c', nch, nt ? "nt   " : "plain", map, group,
                                   load ? (rep == 0 ? " run1" : rep == 1 ? " run2" : " run3") : "",
                                   us, tbs(us));
                        }
    }
    if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); return 1; }
    return 0;
}
