// list_kernels.h -- the exclusive scan of per-row counts into Arrow int32 offsets, shared by the VCF text parser (gpu_parse.hip),
// the BCF parser (bcf_parse.hip) and the string columns (text_columns.hip): per-workgroup sums (k_list_block_sums) -> one
// workgroup scans them in place (k_list_scan_blocks) -> the consumer's own kernel adds the in-block prefix (list_first_item).
// For list-valued INFO fields the extract kernel leaves, per row, the number of items (0 for a NULL list) and where they are,
// the format's fill kernel parses the items, and k_pack_bits turns the per-item flags into the child validity bitmap; InfoBufs
// holds one INFO key's device buffers in both parsers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace {  // one copy per translation unit

constexpr int LIST_TPB = 256;
// per-workgroup sums of cnt[0 .. n_rows): n_rows = min(*n_rows_p, cap) read from the device (the row count of this slab), or
// n_rows = cap when n_rows_p is null (the count is known on the host)
__global__ __launch_bounds__(LIST_TPB) void k_list_block_sums(const uint32_t* __restrict__ cnt, const unsigned* __restrict__ n_rows_p,
                                                              unsigned cap, unsigned* __restrict__ block_sums) {
  __shared__ unsigned red[LIST_TPB / 64];
  const unsigned n_rows = n_rows_p ? min(*n_rows_p, cap) : cap;
  const unsigned row = blockIdx.x * LIST_TPB + threadIdx.x;
  unsigned c = row < n_rows ? cnt[row] : 0u;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// exclusive scan of `nb` workgroup totals in place; total -> *total_out
// (One workgroup of 256 threads, not 1024: a workgroup starts only when ONE CU has wave slots for all of it, and beside the
//  inflate of the next slab -- 30 of a CU's 32 slots -- sixteen free slots took 0.5-1.3 ms to appear: round 4.)
__global__ __launch_bounds__(256) void k_list_scan_blocks(unsigned* __restrict__ counts, int nb, unsigned* __restrict__ total_out) {
  __shared__ unsigned part[256];
  const int per = (nb + 255) / 256;
  const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
  unsigned s = 0;
  for (int b = b0; b < b1; ++b) s += counts[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned run = threadIdx.x ? part[threadIdx.x - 1] : 0u;
  for (int b = b0; b < b1; ++b) {
    const unsigned c = counts[b];
    counts[b] = run;
    run += c;
  }
  if (threadIdx.x == 255) *total_out = part[255];
}
// row -> first item index: block_offsets[block] + the prefix of the counts inside the block (call with all LIST_TPB threads)
__device__ __forceinline__ unsigned list_first_item(unsigned c, const unsigned* __restrict__ block_offsets) {
  __shared__ unsigned wave_tot[LIST_TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  unsigned base = block_offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  return base + incl - c;
}
// bytes [src, src + n) to dst: 8 at a time (unaligned on both sides: the hardware takes it), the rest one by one.  The span copier of
// the text columns' fill kernels (text_columns.hip) and of the take-rows step (take_rows.hip)
__device__ __forceinline__ void copy_run(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, unsigned n) {
  unsigned i = 0;
  for (; i + 8 <= n; i += 8) {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(src + i), b = *reinterpret_cast<const uint32_t*>(src + i + 4);
    *reinterpret_cast<uint32_t*>(dst + i) = a;
    *reinterpret_cast<uint32_t*>(dst + i + 4) = b;
  }
  for (; i < n; ++i) dst[i] = src[i];
}
// byte-per-item flags -> Arrow validity bitmap (8 items per thread); n = offsets[n_rows], never more than the `cap_items`
// the flag / bitmap buffers were sized for (a slab whose items do not fit is handed back to the host decoder by the fill
// kernel's exception count: nothing past the buffers may be touched on the way there)
__global__ __launch_bounds__(256) void k_pack_bits(const uint8_t* __restrict__ flags, const int32_t* __restrict__ offsets,
                                                   const unsigned* __restrict__ n_rows_p, unsigned cap, unsigned cap_items,
                                                   uint8_t* __restrict__ bitmap) {
  const unsigned n = min((unsigned)offsets[min(*n_rows_p, cap)], cap_items);
  for (unsigned b = blockIdx.x * 256 + threadIdx.x; b * 8 < n; b += gridDim.x * 256) {
    unsigned v = 0;
    for (unsigned k = 0; k < 8 && b * 8 + k < n; ++k) v |= (unsigned)(flags[b * 8 + k] & 1) << k;
    bitmap[b] = (uint8_t)v;
  }
}

// counts -> scanned block sums (`nb` workgroups of LIST_TPB rows; the total -> *total): the first two launches of every offsets scan
inline void launch_list_scan(hipStream_t s, const uint32_t* cnt, const unsigned* n_rows_p, unsigned cap, int nb, unsigned* block_sums,
                             unsigned* total) {
  hipLaunchKernelGGL(k_list_block_sums, dim3(nb), dim3(LIST_TPB), 0, s, cnt, n_rows_p, cap, block_sums);
  hipLaunchKernelGGL(k_list_scan_blocks, dim3(1), dim3(256), 0, s, block_sums, nb, total);
}

// One INFO key's device buffers.  Number=1 kinds: the 4-byte column `value` and its validity bitmap `valid` (VCF: bytes, BCF: 32-bit
// words).  List kinds ('F' / 'I'): per row where the value is and how many items it has (VCF 's' keys: the value text), the Arrow
// offsets [rows + 1], the per-item flags, the child validity bitmap and the items.
struct InfoBufs {
  float* value = nullptr;
  void* valid = nullptr;
  uint32_t *lv_off = nullptr, *lv_cnt = nullptr;
  int32_t* offsets = nullptr;
  uint8_t *item_flags = nullptr, *item_bits = nullptr;
  float* items = nullptr;
  void take_list(PoolBufs& b, size_t rows, size_t cap_items) {
    lv_off = b.take<uint32_t>(rows * 4);
    lv_cnt = b.take<uint32_t>(rows * 4);
    offsets = b.take<int32_t>((rows + 1) * 4);
    item_flags = b.take<uint8_t>(cap_items);
    item_bits = b.take<uint8_t>(cap_items / 8 + 64);
    items = b.take<float>(cap_items * 4);
  }
  // the per-item flags -> the child validity bitmap, behind the format's fill kernel
  void pack_bits(hipStream_t s, const unsigned* n_rows_p, unsigned cap, unsigned cap_items) const {
    hipLaunchKernelGGL(k_pack_bits, dim3(1024), dim3(256), 0, s, item_flags, offsets, n_rows_p, cap, cap_items, item_bits);
  }
};

}  // namespace
