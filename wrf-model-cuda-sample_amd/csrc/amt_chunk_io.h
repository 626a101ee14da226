// amt_chunk_io.h -- a 16-byte chunk of a contiguous run into the lanes of one vector and back: what the streaming kernels
// (amt_sumflux.hip, amt_stage.hip, amt_bdy.hip, amt_moments.hip) share on the device, so that each states its arithmetic
// once, on the lanes of a vector, whichever way the chunk moves.  The CALLER decides `wide` -- a whole chunk (cnt == kPer)
// whose address lies on a 16-byte boundary -- and the helpers never widen an access on their own; otherwise the chunk moves
// element by element, the lanes behind `cnt` are not read and hold zero, and what is computed in them is never stored.
// amt_p_rho_load / _store (amt_p_rho_kernel.h) are the same pair over a wave-uniform base with a 32-bit lane offset.
// Host and device, no HIP call: tests/chunk_io_check.cpp runs both ways on the host, in buffers that end with the chunk.
#pragma once

#include "amt_chunk_index.h"

// what a lane moves at once: 16 bytes
template <typename T> struct AmtVec16;
template <> struct AmtVec16<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct AmtVec16<double> { typedef double type __attribute__((ext_vector_type(2))); };

template <typename T>
AMT_CHUNK_INDEX_FN typename AmtVec16<T>::type amt_chunk_load(const T *p, bool wide, int cnt)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    if (wide) return *reinterpret_cast<const V *>(p);
    V v;
#pragma unroll
    for (int i = 0; i < kPer; ++i) v[i] = i < cnt ? p[i] : T(0);
    return v;
}

template <typename T>
AMT_CHUNK_INDEX_FN void amt_chunk_store(T *p, bool wide, int cnt, typename AmtVec16<T>::type v)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    if (wide) {
        *reinterpret_cast<V *>(p) = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i)
        if (i < cnt) p[i] = v[i];
}
