// ffpa_kvcache_append_rows.h — what the append kernels (ffpa_kvcache_append.hip, ffpa_kvcache_append_varlen.hip) share on the device: the 16-byte vector types
// and the load / rotate / store of one lane's unit of a token row's heads.  In an anonymous namespace (everything here is inlined into the kernels:
// no symbol leaves a TU), so the attention kernels' objects see nothing of it.
#pragma once
#include "ffpa_kvcache_append.h"

namespace ffpa {
namespace {

template <typename T>
struct Vec {
  typedef T v8 __attribute__((ext_vector_type(8)));
  typedef T v4 __attribute__((ext_vector_type(4)));
};

// Unit [lo, lo + 8) (+ [hi, hi + 8) in the NeoX form) of heads h0, h0 + hstep, ... < H of one token row, rotated (or copied) in two steps: load() issues
// every load (the unit's cos / sin of the position, then the heads' rows), store() rotates and writes.  The kernel issues the loads of its K row, its q row
// and its V chunk before the first store, so a lane waits for memory once.
template <typename T, bool INTERLEAVED>
struct HeadRows {
  using v8 = typename Vec<T>::v8;
  using v4 = typename Vec<T>::v4;
  static constexpr int HPL = kAppendHeadsPerLane;
  v8 x[HPL], y[HPL];
  v8 cv, sv;   // NeoX: pairs lo ... lo + 7
  v4 cv4, sv4;  // interleaved: pairs lo / 2 ... lo / 2 + 3

  __device__ __forceinline__ void load(const T* src, int64_t src_hs, int H, int h0, int hstep, int lo, int hi, bool rot, const T* cs, const T* sn) {
    if (rot) {
      if constexpr (INTERLEAVED) {
        cv4 = *(const v4*)(cs + lo / 2), sv4 = *(const v4*)(sn + lo / 2);
      } else {
        cv = *(const v8*)(cs + lo), sv = *(const v8*)(sn + lo);
      }
    }
#pragma unroll
    for (int j = 0; j < HPL; ++j) {
      const int h = h0 + j * hstep;
      if (h < H) {
        x[j] = *(const v8*)(src + h * src_hs + lo);
        if (!INTERLEAVED && rot) y[j] = *(const v8*)(src + h * src_hs + hi);
      }
    }
  }

  __device__ __forceinline__ void store(T* dst, int64_t dst_hs, int H, int h0, int hstep, int lo, int hi, bool rot) const {
#pragma clang fp contract(off)
    float c[8], s[8];
    if (rot) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (INTERLEAVED) {
          if (e < 4) c[e] = (float)cv4[e], s[e] = (float)sv4[e];
        } else {
          c[e] = (float)cv[e], s[e] = (float)sv[e];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < HPL; ++j) {
      const int h = h0 + j * hstep;
      if (h >= H) continue;
      T* d = dst + h * dst_hs;
      if (!rot) {
        *(v8*)(d + lo) = x[j];
        continue;
      }
      v8 ox, oy;
      if constexpr (INTERLEAVED) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float x0 = (float)x[j][2 * p], x1 = (float)x[j][2 * p + 1];
          ox[2 * p] = (T)(x0 * c[p] - x1 * s[p]);
          ox[2 * p + 1] = (T)(x1 * c[p] + x0 * s[p]);
        }
        *(v8*)(d + lo) = ox;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float x0 = (float)x[j][e], x1 = (float)y[j][e];
          ox[e] = (T)(x0 * c[e] - x1 * s[e]);
          oy[e] = (T)(x1 * c[e] + x0 * s[e]);
        }
        *(v8*)(d + lo) = ox;
        *(v8*)(d + hi) = oy;
      }
    }
  }
};

}  // namespace
}  // namespace ffpa
