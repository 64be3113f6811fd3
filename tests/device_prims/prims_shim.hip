// Test shim for ipc_amd/csrc/device_prims.h (tests/test_gpu_device_prims.py): C entry points that launch one-line kernels around the shared helpers.
// Host pointers in, host pointers out; every entry returns a hipError_t (0 = ok).  Compiled with -ffp-contract=off like the units that scale and accumulate.
#include "device_prims.h"
#include <vector>

using namespace ipcgpu::prims;

namespace {
constexpr int BLOCK = 256;

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n;
    hipError_t err;
    Dev(const T* host, size_t count) : n(count)
    {
        err = hipMalloc(&p, (n ? n : 1) * sizeof(T));
        if (err == hipSuccess && host && n) err = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t get(T* host) { return n ? hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipDeviceSynchronize(); }
    ~Dev() { (void)hipFree(p); }
};

// op: 0 wave_sum, 1 wave_min, 2 wave_max (out[wave] from lane 0), 3 wave_sum_all (out[lane] from every lane); lanes past n hold pad
template <class T>
__global__ __launch_bounds__(64) void k_wave(int op, const T* __restrict__ in, int n, T pad, T* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    T x = i < n ? in[i] : pad;
    if (op == 0) x = wave_sum(x);
    else if (op == 1) x = wave_min(x);
    else if (op == 2) x = wave_max(x);
    else x = wave_sum_all(x);
    if (op == 3) out[i] = x;
    else if (threadIdx.x == 0) out[blockIdx.x] = x;
}
__global__ __launch_bounds__(BLOCK) void k_block_partials(const double* __restrict__ in, int n, double* __restrict__ partial)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    store_block_sum<BLOCK>(i < n ? in[i] : 0.0, partial);
}
__global__ void k_row_off(int L, int* __restrict__ out)
{
    if (threadIdx.x < 3) out[threadIdx.x] = block_row_off(threadIdx.x, L);
}
// out[q] = find_block over the first CSR row of node rn[q] for neighbour cn[q]
__global__ void k_find_block(int n, const int* __restrict__ ia, const int* __restrict__ ja, const int* __restrict__ rn, const int* __restrict__ cn, int* __restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = find_block(ja, ia[3 * rn[q]] + 3, ia[3 * rn[q] + 1], cn[q]);
}

template <class T>
int run_wave(int op, const T* in, int n, T pad, T* out)
{
    const int nw = (n + 63) / 64;
    Dev<T> dIn(in, n), dOut(nullptr, op == 3 ? 64 * (size_t)nw : nw);
    if (dIn.err != hipSuccess || dOut.err != hipSuccess) return 1000;
    if (nw) hipLaunchKernelGGL(k_wave<T>, dim3(nw), dim3(64), 0, 0, op, dIn.p, n, pad, dOut.p);
    if (hipGetLastError() != hipSuccess) return 1001;
    return (int)dOut.get(out);
}
} // namespace

extern "C" {
// out: (n + 63) / 64 values for op 0 .. 2, 64 per wave for op 3
int prims_wave_f64(int op, const double* in, int n, double pad, double* out) { return run_wave<double>(op, in, n, pad, out); }
int prims_wave_i32(int op, const int* in, int n, int pad, int* out) { return run_wave<int>(op, in, n, pad, out); }

// partial[nblk(n)] = store_block_sum<256> over workgroups of 256 items (0.0 past n)
int prims_block_partials(const double* in, int n, double* partial)
{
    const int nb = nblk(n, BLOCK);
    Dev<double> dIn(in, n), dPart(nullptr, nb);
    if (dIn.err != hipSuccess || dPart.err != hipSuccess) return 1000;
    if (nb) hipLaunchKernelGGL(k_block_partials, dim3(nb), dim3(BLOCK), 0, 0, dIn.p, n, dPart.p);
    if (hipGetLastError() != hipSuccess) return 1001;
    return (int)dPart.get(partial);
}
// the plain reduce kernel over n partials; out[0] holds the value accumulated into and receives the result
int prims_reduce(const double* partial, int n, double scale, int accumulate, double* out)
{
    Dev<double> dPart(partial, n), dOut(out, 1);
    if (dPart.err != hipSuccess || dOut.err != hipSuccess) return 1000;
    launch_reduce_partials(dPart.p, n, scale, accumulate != 0, dOut.p, 0);
    if (hipGetLastError() != hipSuccess) return 1001;
    return (int)dOut.get(out);
}
int prims_block_row_off(int L, int* out3)
{
    Dev<int> dOut(nullptr, 3);
    if (dOut.err != hipSuccess) return 1000;
    hipLaunchKernelGGL(k_row_off, dim3(1), dim3(64), 0, 0, L, dOut.p);
    if (hipGetLastError() != hipSuccess) return 1001;
    return (int)dOut.get(out3);
}
// nRows: scalar rows of the upper CSR (ia has nRows + 1 entries, ja ia[nRows]); n queries (rn[q] < cn[q] < nRows / 3)
int prims_find_block(int nRows, const int* ia, const int* ja, int n, const int* rn, const int* cn, int* out)
{
    Dev<int> dIa(ia, nRows + 1), dJa(ja, ia[nRows]), dRn(rn, n), dCn(cn, n), dOut(nullptr, n);
    if (dIa.err != hipSuccess || dJa.err != hipSuccess || dRn.err != hipSuccess || dCn.err != hipSuccess || dOut.err != hipSuccess) return 1000;
    if (n) hipLaunchKernelGGL(k_find_block, dim3(nblk(n, 64)), dim3(64), 0, 0, n, dIa.p, dJa.p, dRn.p, dCn.p, dOut.p);
    if (hipGetLastError() != hipSuccess) return 1001;
    return (int)dOut.get(out);
}
int prims_nblk(long long n, int block) { return nblk(n, block); }
}
