// What the two selections share (tmpnn_hits.hip: tmpnn_select_hits; tmpnn_variant_hits.hip: tmpnn_select_variant_hits): the 64-bit
// key's value word, and the k smallest of up to 8 192 keys in one 64 KB LDS image by a workgroup of 512 threads. Integer compares
// only. The network and its LDS access pattern are described at the top of tmpnn_hits.hip.
#pragma once
#include <stdint.h>

#define HITS_THREADS 512
#define HITS_B 256                  // residues per stage-1 block
#define HITS_MAX_KEYS 8192          // 64 KB of LDS
#define HITS_MAX_K 256
#define HITS_CYS 1                  // 'C' in ALPHABET = ACDEFGHIKLMNPQRSTVWYX

typedef unsigned long long hkey_t;
#define HITS_NONE (~(hkey_t)0)

__host__ __device__ static inline uint32_t hits_ord(uint32_t b) {
    if (b == 0x80000000u) b = 0;
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// one compare-exchange of the network: ascending when `up`
__device__ __forceinline__ void hits_cx(hkey_t *keys, int lo, int hi, bool up) {
    const hkey_t x = keys[lo], y = keys[hi];
    if ((x > y) == up) {
        keys[lo] = y;
        keys[hi] = x;
    }
}

// the m smallest of keys[0 .. n) into keys[0 .. m), ascending, by the whole workgroup; n >= m >= 2 powers of two, n <= HITS_MAX_KEYS;
// the rest of keys[] is left in no particular order; ends behind a barrier
__device__ __forceinline__ void hits_topk(hkey_t *keys, int n, int m) {
    const int tid = threadIdx.x, half = n >> 1;
    for (int size = 2; size <= m; size <<= 1) {                       // (1) chunks of m, ascending and descending in turn
        for (int d = size >> 1; d > 0; d >>= 1) {
            for (int i = tid; i < half; i += HITS_THREADS) {
                const int lo = ((i & ~(d - 1)) << 1) | (i & (d - 1));
                hits_cx(keys, lo, lo | d, (lo & size) == 0);
            }
            __syncthreads();
        }
    }
    const int lgm = __ffs(m) - 1, hm = m >> 1;
    for (int s = 1; s * m < n; s <<= 1) {                             // (2) live chunks sit s chunks apart; n / (s m) of them, an even number
        const int pairs = n / (s * m) >> 1;
        for (int idx = tid; idx < pairs * m; idx += HITS_THREADS) {   // chunk 2 q (ascending) <- min with chunk 2 q + 1 (descending)
            const int a = ((idx >> lgm) * 2 * s << lgm) + (idx & (m - 1)), b = a + (s << lgm);
            const hkey_t x = keys[a], y = keys[b];
            if (y < x) keys[a] = y;
        }
        __syncthreads();
        for (int d = hm; d > 0; d >>= 1) {                            // survivor r, at chunk 2 s r, is bitonic: merge it, ascending for even r
            for (int idx = tid; idx < pairs * hm; idx += HITS_THREADS) {
                const int r = idx >> (lgm - 1), i = idx & (hm - 1);
                const int lo = (r * 2 * s << lgm) + (((i & ~(d - 1)) << 1) | (i & (d - 1)));
                hits_cx(keys, lo, lo + d, (r & 1) == 0);
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int hits_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}
