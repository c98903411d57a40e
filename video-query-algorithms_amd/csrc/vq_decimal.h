// Decimal text -> binary64, and binary64 -> the storage types of a feature database: the arithmetic the device loader of feature
// CSV files (csrc/vq_csv.hip) and the host (csrc/host/vq_csv_read.cc, tests/sanitize_csv) share.  No HIP include of its own: under
// hipcc every function is __host__ __device__, under a plain C++ compiler it is an ordinary inline function.
//
// What a field of the reference's feature files is (tsn/feature_csv.py): str(numpy.float64) -- at most 17 significant digits, fixed or
// d.ddde-XX.  vq_dec_scan reads such a field into (sign, w, q): value = +-w * 10^q with w < 10^19.  vq_dec_to_double turns (w, q)
// into the correctly rounded binary64 (round to nearest, ties to even -- what Python's float() returns) with one 64 x 64 -> 128
// multiplication by a tabulated 128-bit approximation of 5^q (a second one when the first leaves the rounding open), after
// Eisel and Lemire ("Number parsing at a gigabyte per second", 2021): the product's top bits are the significand, q alone gives the
// binary exponent.  When even the 192-bit product cannot tell which side of a rounding boundary the value is on the function says so
// (VQ_DEC_UNDECIDED) and the caller asks the host's parser; the same for more than 19 significant digits.
#pragma once
#include <stdint.h>

#include "vq_pow5_table.h"

#if defined(__HIPCC__)
#define VQ_HD __host__ __device__
#else
#define VQ_HD
#endif

enum {
    VQ_DEC_OK = 0,
    VQ_DEC_ASK_HOST = 1,      // the scanner: outside the fast-path grammar (spaces, inf, nan, anything malformed)
    VQ_DEC_UNDECIDED = 2      // the conversion: more than 19 significant digits, or the truncated product cannot settle the rounding
};

struct vq_dec_field {
    uint64_t w;         // the first (up to 19) significant digits as an integer
    int32_t q;          // decimal exponent of w's last digit
    int32_t digits;     // significant digits met (w holds min(digits, 19) of them)
    int32_t neg;
    int32_t status;     // VQ_DEC_OK / VQ_DEC_ASK_HOST
};

// high and low 64 bits of a * b
VQ_HD inline void vq_mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    *lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    *hi = (uint64_t)(p >> 64);
    *lo = (uint64_t)p;
#endif
}

VQ_HD inline int vq_clz64(uint64_t x) {      // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// [begin, end) -> (sign, w, q).  Fast-path grammar: [+-]? digits [. digits*]? ([eE][+-]?digits)?  or  [+-]? . digits ([eE]...)?
// Reads no byte outside [begin, end).  Everything else: status VQ_DEC_ASK_HOST.
VQ_HD inline vq_dec_field vq_dec_scan(const char* begin, const char* end) {
    vq_dec_field f;
    f.w = 0;
    f.q = 0;
    f.digits = 0;
    f.neg = 0;
    f.status = VQ_DEC_ASK_HOST;
    const char* p = begin;
    if (p < end && (*p == '+' || *p == '-')) {
        f.neg = *p == '-';
        ++p;
    }
    bool any = false;
    for (; p < end && *p >= '0' && *p <= '9'; ++p) {
        any = true;
        const unsigned d = (unsigned)(*p - '0');
        if (f.digits > 0 || d != 0) {
            if (f.digits < 19) f.w = f.w * 10 + d;
            ++f.digits;
        }
    }
    if (p < end && *p == '.') {
        ++p;
        for (; p < end && *p >= '0' && *p <= '9'; ++p) {
            any = true;
            const unsigned d = (unsigned)(*p - '0');
            if (f.digits > 0 || d != 0) {
                if (f.digits < 19) f.w = f.w * 10 + d;
                ++f.digits;
            }
            if (f.q > -100000) --f.q;
        }
    }
    if (!any) return f;
    if (p < end && (*p == 'e' || *p == 'E')) {
        ++p;
        bool eneg = false;
        if (p < end && (*p == '+' || *p == '-')) {
            eneg = *p == '-';
            ++p;
        }
        if (!(p < end && *p >= '0' && *p <= '9')) return f;
        int32_t ex = 0;
        for (; p < end && *p >= '0' && *p <= '9'; ++p)
            if (ex < 100000) ex = ex * 10 + (*p - '0');
        f.q += eneg ? -ex : ex;
    }
    if (p != end) return f;
    f.status = VQ_DEC_OK;
    return f;
}

// +-w * 10^q (w holds all of `digits` significant digits, i.e. digits <= 19) -> the bits of the nearest binary64, ties to even;
// subnormals, +-0, overflow to +-inf and underflow to +-0 as strtod / Python's float().  VQ_DEC_OK or VQ_DEC_UNDECIDED.
VQ_HD inline int vq_dec_to_double(uint64_t w, int32_t q, int32_t digits, int32_t neg, uint64_t* bits) {
    const uint64_t sign = neg ? 0x8000000000000000ull : 0ull;
    if (digits > 19) return VQ_DEC_UNDECIDED;
    if (w == 0 || q < VQ_POW5_QMIN) {                    // w < 10^19 < 2^64 and 10^-343 * 2^64 is below half the smallest subnormal
        *bits = sign;
        return VQ_DEC_OK;
    }
    if (q > VQ_POW5_QMAX) {
        *bits = sign | 0x7FF0000000000000ull;
        return VQ_DEC_OK;
    }
    const int lz = vq_clz64(w);
    w <<= lz;
    const uint64_t* t = vq_pow5_128[q - VQ_POW5_QMIN];
    uint64_t hi, lo;
    vq_mul64(w, t[0], &hi, &lo);
    if ((hi & 0x1FF) == 0x1FF) {                         // the 9 bits below the 53 + 1 + 1 kept are all ones: the low word may carry into them
        uint64_t hi2, lo2;
        vq_mul64(w, t[1], &hi2, &lo2);
        lo += hi2;
        if (hi2 > lo) ++hi;
        if (lo == 0xFFFFFFFFFFFFFFFFull && (q < -27 || q > 55)) return VQ_DEC_UNDECIDED;     // 5^q is not exact in 128 bits there
    }
    const int upper = (int)(hi >> 63);
    uint64_t m = hi >> (upper + 9);                      // 54 bits: the significand and one rounding bit
    // floor(q * log2(10)) = (217706 * q) >> 16 for |q| <= 342; +63 for the 64-bit significand
    int32_t e2 = (int32_t)((217706 * (int64_t)q) >> 16) + 63 + upper - lz + 1023;
    if (e2 <= 0) {                                       // subnormal (or zero)
        if (-e2 + 1 >= 64) {
            *bits = sign;
            return VQ_DEC_OK;
        }
        m >>= -e2 + 1;
        m += m & 1;
        m >>= 1;
        // rounding may carry into the smallest normal: then the exponent field is 1 and the hidden bit must go
        *bits = sign | (m < (1ull << 52) ? m : ((1ull << 52) | (m & ((1ull << 52) - 1))));
        return VQ_DEC_OK;
    }
    // an exact half-way case (only where 5^q is exact and small: -4 <= q <= 23): the bits that were shifted out are all zero
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << (upper + 9)) == hi) m &= ~1ull;      // a tie with an even significand: stay
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {
        m = 1ull << 52;
        ++e2;
    }
    m &= ~(1ull << 52);
    if (e2 >= 0x7FF) {
        *bits = sign | 0x7FF0000000000000ull;
        return VQ_DEC_OK;
    }
    *bits = sign | ((uint64_t)e2 << 52) | m;
    return VQ_DEC_OK;
}

// scanner + conversion: VQ_DEC_OK with the bits, or the reason the host has to look at the field
VQ_HD inline int vq_dec_parse(const char* begin, const char* end, uint64_t* bits) {
    const vq_dec_field f = vq_dec_scan(begin, end);
    if (f.status != VQ_DEC_OK) return f.status;
    return vq_dec_to_double(f.w, f.q, f.digits, f.neg, bits);
}

// ---- storage conversions: ONE round-to-nearest-even step from the double ------------------------------------------------------
// *overflow is set when a FINITE double becomes +-inf in the target type.

// binary64 -> binary32 bits, like numpy's astype(float32): the overflowed value is stored as inf
VQ_HD inline uint32_t vq_f64_to_f32_bits(uint64_t d, int* overflow) {
    const uint32_t sign = (uint32_t)(d >> 32) & 0x80000000u;
    const int e = (int)((d >> 52) & 0x7FF);
    const uint64_t frac = d & ((1ull << 52) - 1);
    *overflow = 0;
    if (e == 0x7FF) return sign | 0x7F800000u | (frac ? (0x00400000u | (uint32_t)(frac >> 29)) : 0u);
    const int E = e - 1023;
    if (E > 127) {
        *overflow = 1;
        return sign | 0x7F800000u;
    }
    uint32_t r;
    uint64_t rem, half;
    if (E >= -126) {
        r = ((uint32_t)(E + 127) << 23) | (uint32_t)(frac >> 29);
        rem = frac & ((1ull << 29) - 1);
        half = 1ull << 28;
    } else if (E >= -150 && e != 0) {
        const int shift = 29 + (-126 - E);               // 30 .. 53
        const uint64_t full = frac | (1ull << 52);
        r = (uint32_t)(full >> shift);
        rem = full & ((1ull << shift) - 1);
        half = 1ull << (shift - 1);
    } else {
        return sign;                                     // below half the smallest subnormal float (binary64 subnormals included)
    }
    if (rem > half || (rem == half && (r & 1))) ++r;     // a carry runs into the exponent field: the next binade, or inf
    if (r == 0x7F800000u) *overflow = 1;
    return sign | r;
}

// binary64 -> binary16 bits, like numpy's astype(float16) (never through float: that would round twice)
VQ_HD inline uint16_t vq_f64_to_f16_bits(uint64_t d, int* overflow) {
    const uint16_t sign = (uint16_t)((d >> 48) & 0x8000u);
    const int e = (int)((d >> 52) & 0x7FF);
    const uint64_t frac = d & ((1ull << 52) - 1);
    *overflow = 0;
    if (e == 0x7FF) return (uint16_t)(sign | 0x7C00u | (frac ? (0x0200u | (uint16_t)(frac >> 42)) : 0u));
    const int E = e - 1023;
    if (E > 15) {
        *overflow = 1;
        return (uint16_t)(sign | 0x7C00u);
    }
    uint32_t r;
    uint64_t rem, half;
    if (E >= -14) {
        r = ((uint32_t)(E + 15) << 10) | (uint32_t)(frac >> 42);
        rem = frac & ((1ull << 42) - 1);
        half = 1ull << 41;
    } else if (E >= -25 && e != 0) {
        const int shift = 42 + (-14 - E);                // 43 .. 53
        const uint64_t full = frac | (1ull << 52);
        r = (uint32_t)(full >> shift);
        rem = full & ((1ull << shift) - 1);
        half = 1ull << (shift - 1);
    } else {
        return sign;
    }
    if (rem > half || (rem == half && (r & 1))) ++r;
    if (r == 0x7C00u) *overflow = 1;
    return (uint16_t)(sign | r);
}
