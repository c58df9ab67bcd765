// kernels_map.hip -- the one strided move through a derived handle's position map (PosMap, spmv_internal.hpp): what
// spmv_csr_transpose_gather, spmv_csr_permute_gather / _values and spmv_csr_select_gather / _scatter / _values launch.
//
// `count` arrays of 32-bit words go through the map in one launch, copied as bits: the map is read once, a word per lane, so
// a caller's arrays need no more than the 4-byte alignment of a float (the 16-byte stores of k_tr_gather, kernels_transpose.hip,
// are for the library's own allocations).  Array c starts c * stride words in: a 64-bit product.  The map's entries lie
// below its parent's length by construction; one that does not is never used as an index.
#include "spmv_internal.hpp"

namespace spmv {

namespace {

// gather: dst[c][i] = src[c][map[i]]; SCATTER: dst[c][map[i]] = src[c][i], for i < n.  An entry at or beyond the parent's
// length: ZERO (a gather that writes the whole of dst: transpose, permute, whose parent has n entries too) stores 0,
// otherwise (select: `bound` entries) the word is left as it is.
template <bool SCATTER, bool ZERO>
__global__ __launch_bounds__(kBlock) void k_map_move(int64_t n, int64_t bound, int count, const uint32_t *__restrict__ map,
                                                     const uint32_t *__restrict__ src, int64_t src_stride, uint32_t *__restrict__ dst,
                                                     int64_t dst_stride)
{
    static_assert(!(SCATTER && ZERO), "a scatter has no word to zero for an entry out of range");
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t m = (int64_t)map[i];
    if (!ZERO && m >= bound) return;
    for (int c = 0; c < count; ++c) {
        if (SCATTER) dst[c * dst_stride + m] = src[c * src_stride + i];
        // (bound == n here, and comparing with n leaves the instructions of the kernels this one replaced)
        else if (ZERO) dst[c * dst_stride + i] = m < n ? src[c * src_stride + m] : 0u;
        else dst[c * dst_stride + i] = src[c * src_stride + m];
    }
}

}  // namespace

int map_move(const PosMap &map, int64_t n, bool scatter, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride,
             hipStream_t s)
{
    if (n <= 0) return SPMV_OK;
    const bool zero = map.maker != MapMaker::select;
    const auto kernel = scatter ? k_map_move<true, false> : zero ? k_map_move<false, true> : k_map_move<false, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, map.parent_len, count,
                       (const uint32_t *)map.words.get(), (const uint32_t *)src, src_stride, (uint32_t *)dst, dst_stride);
    return check_launch("k_map_move");
}

}  // namespace spmv
