// amt_chunk_index.h -- work item -> (j, k, first element, element count) of the streaming kernels that cut a box of nk * nj
// runs of `ni` contiguous elements into 16-byte chunks (amt_stage.hip, amt_sumflux.hip).  Work item e counts chunks along a
// run first, then the runs (k, j) = (r % nk, r / nk): e = (j * nk + k) * chunks + c with chunks = ceil(ni / kPer).
// `narrow` -- wave-uniform, total = nk * nj * chunks <= 2^31 - 1 -- takes 32-bit divisions where they suffice; the results are
// the same.  Host and device: tests/chunk_index_check.cpp runs both paths on the host, past 2^32 work items.
#pragma once

#if defined(__HIPCC__)
#define AMT_CHUNK_INDEX_FN __host__ __device__ __forceinline__
#else
#define AMT_CHUNK_INDEX_FN inline
#endif

// j, k: the run; i0: the chunk's first element inside its run; cnt: its elements (the run's last chunk may be short)
struct AmtChunk { long j, k, i0; int cnt; };
template <int kPer>
AMT_CHUNK_INDEX_FN AmtChunk amt_chunk_index(long e, long chunks, long nk, long ni, bool narrow)
{
    long r, j;
    if (narrow) {
        r = (long)((unsigned)e / (unsigned)chunks);
        j = (long)((unsigned)r / (unsigned)nk);
    } else {
        r = e / chunks;
        j = r / nk;
    }
    const long k = r - j * nk;
    const long i0 = (e - r * chunks) * kPer;
    const long left = ni - i0;
    return AmtChunk{j, k, i0, left < kPer ? (int)left : kPer};
}
