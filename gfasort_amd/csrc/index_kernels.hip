// index_kernels.hip — the one-off passes either side of the SGD loop, on the device (rocPRIM for
// the scan and the radix sort; the kernels around them are hand-written):
//   K4  initial positions (src/sgd.rs:286-294): exclusive prefix sum of node lengths
//   K6  path_sgd_sort's sort (src/sgd.rs:665-671): positions -> rank order
// and the reordering of positions between the ABI's order and the device's.  (The index build — the node layout and K3 — is
// index_set_kernels.hip's, for one graph as for many.)
#include "sgd_host.h"
#include "device_memory.h"
#include "sort_key.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace gfs {

// ---- ABI order <-> device order of positions / coordinates ------------------------------------------------
// ABI: x[k] (1D, D = 0) or coords[(k*2 + end)*D + dim] by dense index k; device: x[perm[k]] or the end x dimension planes
// coords[(end*D + dim)*N + perm[k]] (sgd_device.h coord_ptr).  to_device = 1: abi -> dev, else dev -> abi.
__global__ void reorder_positions_kernel(const double *src, double *dst, const uint32_t *perm, uint64_t N, uint32_t D, int to_device) {
    const uint64_t W = D ? 2ull * D : 1ull, total = N * W;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint64_t k = t / W, r = t - k * W;                  // t walks the ABI order; r = end*D + dim
        const uint64_t dev = r * N + perm[k];
        if (to_device) dst[dev] = src[t]; else dst[t] = src[dev];
    }
}
hipError_t reorder_positions_device(const double *d_src, double *d_dst, const uint32_t *d_perm, uint64_t N, uint32_t D,
                                    int to_device, hipStream_t st) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(reorder_positions_kernel, dim3(2048), dim3(256), 0, st, d_src, d_dst, d_perm, N, D, to_device);
    return hipGetLastError();
}

// ---- K4: initial 1D positions (sgd.rs:286-294): exclusive prefix sum of node lengths in node_order ---------
__global__ void widen_len_kernel(const uint32_t *node_len, uint64_t *out, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) out[k] = node_len[k];
}
__global__ void scatter_prefix_kernel(const uint64_t *prefix, const uint32_t *perm, double *x, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        x[perm[k]] = (double)prefix[k];                          // the reference accumulates in usize and converts (sgd.rs:291)
}
// x[perm[k]] = sum of node_len[0..k).  Synchronous.
hipError_t init_positions_device(const uint32_t *d_node_len, const uint32_t *d_perm, double *d_x, uint64_t n) {
    if (n == 0) return hipSuccess;
    Buffer tmp;                                                            // (scope frees them last to first, after the synchronise)
    Array<uint64_t> scan, len;
    hipError_t e;
    if ((e = len.grow(n * 8)) != hipSuccess) return e;
    if ((e = scan.grow(n * 8)) != hipSuccess) return e;
    uint64_t *d_len = len, *d_scan = scan;
    hipLaunchKernelGGL(widen_len_kernel, dim3(1024), dim3(256), 0, 0, d_node_len, d_len, n);
    size_t tmp_bytes = 0;
    e = rocprim::exclusive_scan(nullptr, tmp_bytes, d_len, d_scan, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), 0);
    if (e != hipSuccess) return e;
    if ((e = tmp.grow(tmp_bytes ? tmp_bytes : 8)) != hipSuccess) return e;
    e = rocprim::exclusive_scan(tmp.p, tmp_bytes, d_len, d_scan, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), 0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scatter_prefix_kernel, dim3(1024), dim3(256), 0, 0, d_scan, d_perm, d_x, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipDeviceSynchronize();
}

// ---- K6 (the key of a position: sort_key.h orderable) --------------------------------------------
// keys in DENSE-index order (the device vector is in layout order), so that the stable sort breaks ties by dense index
__global__ void sort_keys_kernel(const double *x_layout, const uint32_t *perm, uint64_t *keys, uint32_t *vals, uint64_t n,
                                 uint64_t stride_doubles) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        keys[k] = orderable(x_layout[(uint64_t)perm[k] * stride_doubles]);
        vals[k] = (uint32_t)k;
    }
}

// d_order_out[r] = dense index of the node of rank r.  d_tmp: 2*n u64 keys + 2*n u32 values.  Synchronous.
hipError_t sort_order_device(const double *d_x_layout, const uint32_t *d_perm, uint64_t n, uint64_t stride_doubles,
                             void *d_tmp, uint32_t **d_order_out) {
    uint64_t *k_in = reinterpret_cast<uint64_t *>(d_tmp), *k_out = k_in + n;
    uint32_t *v_in = reinterpret_cast<uint32_t *>(k_out + n), *v_out = v_in + n;
    hipLaunchKernelGGL(sort_keys_kernel, dim3(1024), dim3(256), 0, 0, d_x_layout, d_perm, k_in, v_in, n, stride_doubles);
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, 64, 0);
    if (e != hipSuccess) return e;
    Buffer d_sort_tmp;                                                     // (freed after the synchronise)
    if ((e = d_sort_tmp.grow(tmp_bytes ? tmp_bytes : 8)) != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(d_sort_tmp.p, tmp_bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, 64, 0);   // stable
    const hipError_t e2 = hipDeviceSynchronize();
    *d_order_out = v_out;
    return e != hipSuccess ? e : e2;
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_index() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sort_keys_kernel));
}

}  // namespace gfs
