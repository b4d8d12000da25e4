// btx_bucket.hip — K14: the gradient bucket of data-parallel training (include/btx.h).  Two multi-tensor launches in
// the style of btx_optim.hip: pack scales every tensor of a step into ONE flat f32 buffer (the operand of the step's single
// all-reduce), unpack copies the reduced slices back.  HBM-bound, 8 B/element.  Built with -ffp-contract=off: the one multiply of
// pack is rounded once (there is nothing to contract it with; the flag pins that).  gfx950 only.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/btx.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BKT_BLOCK = 256;
constexpr int BKT_CHUNK = BTX_OPTIM_CHUNK;  // elements a workgroup owns: 4 x float4 per thread
constexpr int BKT_MAX_ITEMS = 48;           // per launch: the table travels by value in the kernel arguments
static_assert(BKT_CHUNK % (BKT_BLOCK * 4) == 0, "a chunk is a whole number of float4 sweeps");

struct BktItemDev {
  float* t;  // the tensor: read by pack, written by unpack
  float* b;  // its slice of the bucket (bucket + offset)
  uint64_t n;
  uint32_t first_block, pad;
};
struct BktBatchDev {
  BktItemDev it[BKT_MAX_ITEMS];
  int n;
  uint32_t total_blocks;
};

// PACK: b[i] = t[i] * scale;  otherwise t[i] = b[i]
template <bool PACK>
__global__ __launch_bounds__(BKT_BLOCK) void bucket_kernel(const BktBatchDev b, float scale) {
  int i = 0;
  for (int j = 1; j < b.n; ++j)
    if (blockIdx.x >= b.it[j].first_block) i = j;
  const BktItemDev& it = b.it[i];
  const size_t lo = (size_t)(blockIdx.x - it.first_block) * BKT_CHUNK;
  const size_t end = lo + BKT_CHUNK;
  const size_t hi = end < it.n ? end : (size_t)it.n;
  float* __restrict__ T = it.t;
  float* __restrict__ B = it.b;
  size_t k = lo;
  if ((((uintptr_t)T | (uintptr_t)B) & 15) == 0) {  // lo is a multiple of 4: alignment carries over
    const size_t nv = (hi - lo) >> 2;
    for (size_t q = threadIdx.x; q < nv; q += BKT_BLOCK) {
      const size_t e = lo + (q << 2);
      if (PACK) {
        f32x4 v = *(const f32x4*)(T + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * scale;
        *(f32x4*)(B + e) = v;
      } else {
        *(f32x4*)(T + e) = *(const f32x4*)(B + e);
      }
    }
    k = lo + (nv << 2);
  }
  for (size_t e = k + threadIdx.x; e < hi; e += BKT_BLOCK) {  // unaligned items, and the tail of aligned ones
    if (PACK) B[e] = T[e] * scale;
    else T[e] = B[e];
  }
}

int bkt_validate(const BtxBucketItem* items, int n_items, const float* bucket) {
  if (n_items < 0) return BTX_E_SHAPE;
  if (n_items > BTX_OPTIM_MAX_ITEMS) return BTX_E_UNSUPPORTED;
  if (!bucket || (n_items > 0 && !items)) return BTX_E_NULL;
  if ((uintptr_t)bucket & 3) return BTX_E_ALIGN;
  for (int i = 0; i < n_items; ++i) {
    const BtxBucketItem& s = items[i];
    if (s.n < 0 || s.offset < 0) return BTX_E_SHAPE;
    if (s.n == 0) continue;
    if ((uint64_t)s.n > 0x7fffffffull * BKT_CHUNK) return BTX_E_UNSUPPORTED;  // more chunks than the grid of one launch
    if (!s.src) return BTX_E_NULL;
    if ((uintptr_t)s.src & 3) return BTX_E_ALIGN;
  }
  return 0;
}

// the next table of at most BKT_MAX_ITEMS non-empty items starting at *pos; false when none is left
bool bkt_next_batch(const BtxBucketItem* items, int n_items, float* bucket, int* pos, BktBatchDev* b) {
  memset(b, 0, sizeof(*b));
  uint32_t blocks = 0;
  int i = *pos;
  for (; i < n_items && b->n < BKT_MAX_ITEMS; ++i) {
    const BtxBucketItem& s = items[i];
    if (s.n == 0) continue;
    const uint64_t nb = ((uint64_t)s.n + BKT_CHUNK - 1) / BKT_CHUNK;
    if (blocks + nb > 0x7fffffffull) break;  // the grid of one launch: the rest goes to the next table (one item always fits)
    BktItemDev& it = b->it[b->n++];
    // unpack writes through src: BtxBucketItem declares it const because pack, the common direction, only reads it
    it.t = const_cast<float*>(s.src); it.b = bucket + s.offset; it.n = (uint64_t)s.n; it.first_block = blocks;
    blocks += (uint32_t)nb;
  }
  *pos = i;
  b->total_blocks = blocks;
  return b->n > 0;
}

template <bool PACK>
int bkt_run(const BtxBucketItem* items, int n_items, float scale, float* bucket, void* stream) {
  const int rc = bkt_validate(items, n_items, bucket);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  BktBatchDev b;
  bool any = false;
  for (int pos = 0; bkt_next_batch(items, n_items, bucket, &pos, &b); any = true)
    hipLaunchKernelGGL(bucket_kernel<PACK>, dim3(b.total_blocks), dim3(BKT_BLOCK), 0, st, b, scale);
  return any ? (int)hipGetLastError() : 0;
}

}  // namespace

extern "C" {

int btx_bucket_pack(const BtxBucketItem* items, int n_items, float scale, float* bucket, void* stream) {
  return bkt_run<true>(items, n_items, scale, bucket, stream);
}

int btx_bucket_unpack(const BtxBucketItem* items, int n_items, const float* bucket, void* stream) {
  return bkt_run<false>(items, n_items, 1.0f, const_cast<float*>(bucket), stream);  // the bucket is only read (PACK == false)
}

}  // extern "C"
