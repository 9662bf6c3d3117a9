// Does v_lshlrev_b64 misread a per-lane shift amount held in v15, the last VGPR of a wave that owns 16?  Two kernels of
// 16 VGPRs that differ only in the register of the amount.  csrc/cloud.h builds its keys from 32-bit shifts because of
// what this prints on an MI355X.
//     hipcc --offload-arch=gfx950 -O3 -o probe_shift64 tools/probe_shift64.hip && ./probe_shift64
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>
__global__ __launch_bounds__(256) void probe_hi(const uint32_t *amt, const uint32_t *val, uint32_t *lo, uint32_t *hi, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t a = amt[i], v = val[i], rl, rh;
    asm volatile("v_mov_b32 v15, %2\n\tv_mov_b32 v10, %3\n\tv_mov_b32 v11, 0\n\ts_nop 4\n\tv_lshlrev_b64 v[12:13], v15, v[10:11]\n\ts_nop 4\n\t"
                 "v_mov_b32 %0, v12\n\tv_mov_b32 %1, v13\n\t" : "=v"(rl), "=v"(rh) : "v"(a), "v"(v) : "v10", "v11", "v12", "v13", "v15");
    lo[i] = rl; hi[i] = rh;
}
__global__ __launch_bounds__(256) void probe_mid(const uint32_t *amt, const uint32_t *val, uint32_t *lo, uint32_t *hi, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t a = amt[i], v = val[i], rl, rh;
    asm volatile("v_mov_b32 v14, %2\n\tv_mov_b32 v10, %3\n\tv_mov_b32 v11, 0\n\ts_nop 4\n\tv_lshlrev_b64 v[12:13], v14, v[10:11]\n\ts_nop 4\n\t"
                 "v_mov_b32 %0, v12\n\tv_mov_b32 %1, v13\n\t" : "=v"(rl), "=v"(rh) : "v"(a), "v"(v) : "v10", "v11", "v12", "v13", "v14", "v15");
    lo[i] = rl; hi[i] = rh;
}
int main() {
    const int n = 307200;
    std::vector<uint32_t> amt(n), val(n), lo(n), hi(n);
    for (int i = 0; i < n; ++i) { amt[i] = 6; val[i] = (uint32_t)(i % 61); }
    uint32_t *da, *dv, *dl, *dh;
    if (hipMalloc(&da, n * 4) || hipMalloc(&dv, n * 4) || hipMalloc(&dl, n * 4) || hipMalloc(&dh, n * 4)) return 2;
    hipMemcpy(da, amt.data(), n * 4, hipMemcpyHostToDevice);
    hipMemcpy(dv, val.data(), n * 4, hipMemcpyHostToDevice);
    for (int which = 0; which < 2; ++which) {
        long bad = 0, zero_shift = 0;
        for (int rep = 0; rep < 200; ++rep) {
            if (which == 0) hipLaunchKernelGGL(probe_hi, dim3((n + 255) / 256), dim3(256), 0, 0, da, dv, dl, dh, n);
            else hipLaunchKernelGGL(probe_mid, dim3((n + 255) / 256), dim3(256), 0, 0, da, dv, dl, dh, n);
            if (hipMemcpy(lo.data(), dl, n * 4, hipMemcpyDeviceToHost) || hipMemcpy(hi.data(), dh, n * 4, hipMemcpyDeviceToHost)) return 3;
            for (int i = 0; i < n; ++i) {
                const uint64_t got = ((uint64_t)hi[i] << 32) | lo[i], want = (uint64_t)val[i] << 6;
                if (got != want) { ++bad; if (got == val[i]) ++zero_shift; }
            }
        }
        printf("amount in %s: %ld wrong results in 200 launches of %d lanes (%ld of them = a shift of 0)\n", which == 0 ? "v15" : "v14", bad, n, zero_shift);
    }
    return 0;
}
