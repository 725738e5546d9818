// extents_point.h — the per-point arithmetic of pgx_instance_extents (extents.hip), HIP-free: a point's coordinates in its instance's
// frame, the sector rule S, the occupancy bins and the order-preserving double <-> u64 key.  The kernels run these lines per lane,
// tests/emu/extents_driver.cpp runs the same lines point by point on the CPU.  include/pgx.h states the contract these
// lines implement; tests/extents_model.py restates it in numpy from that text.
//
// All FP64.  The translation units that include this header are compiled with -ffp-contract=off: no product here may fuse with a sum.
// Division and square root are the IEEE ones; every dot product is the left fold (a0 b0 + a1 b1) + a2 b2.
//
// WHY EVERYTHING IS AN INTEGER REDUCTION.  An instance's row of the table is seven u64 slots and every slot is updated by ONE of
//   add (the count), max (the bounds, as keys), or (the sector masks)
// all three associative and commutative on integers, all three with identity 0: the table starts as zeros, partial tables (a wave's
// registers, a workgroup's LDS) merge by the same three operations, and the result does not depend on which lane ran when.  The
// minimum of a coordinate is kept as the maximum of the INVERTED key, so no slot needs a non-zero start.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PGX_EXT_HD __host__ __device__ __forceinline__
#else
#define PGX_EXT_HD inline
#endif

namespace pgx {

constexpr int kExtFrame = 15;   // doubles per frame row: kind, o[3], g[3], u[3], v[3], R, r (PGX_EXTENTS_FRAME)
// the slots of an instance's table row
enum { EXT_COUNT = 0, EXT_HI_A = 1, EXT_LO_A = 2, EXT_HI_B = 3, EXT_LO_B = 4, EXT_SEC_A = 5, EXT_SEC_B = 6, EXT_SLOTS = 7 };
enum { EXT_UNUSED = 0, EXT_LINEAR = 1, EXT_ANGULAR = 2 };

struct ExtPoint {   // a live point's two coordinates
    int mode[2];    // EXT_UNUSED / EXT_LINEAR / EXT_ANGULAR
    double c[2];    // the linear coordinate, canonicalised (never -0)
    int s[2];       // the angular coordinate's sector, 0..63
};

struct ExtAcc {     // what one point - or a merged set of points of ONE instance - adds to the instance's row; all zeros adds nothing
    uint64_t v[EXT_SLOTS];
};

PGX_EXT_HD uint64_t ext_bits(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

PGX_EXT_HD bool ext_finite(double x) { return (ext_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// finite doubles (and the infinities) -> u64, strictly increasing; never 0, and never ~0: both a key and an inverted key are > 0
PGX_EXT_HD uint64_t ext_key(double x)
{
    const uint64_t b = ext_bits(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

PGX_EXT_HD double ext_unkey(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}

PGX_EXT_HD double ext_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// S(x, y): the sector, of 64, of the direction (x, y); x and y finite and not both zero.  The thresholds are tan(k pi / 32), k = 1..7.
PGX_EXT_HD int ext_sector(double x, double y)
{
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const bool swap = ay > ax;
    const double t = swap ? ax / ay : ay / ax;
    const int s = (t >= 0.09849140335716425) + (t >= 0.198912367379658) + (t >= 0.3033466836073424) + (t >= 0.41421356237309503) +
                  (t >= 0.5345111359507916) + (t >= 0.6681786379192989) + (t >= 0.8206787908286602);
    const int q = swap ? 15 - s : s;
    if (y >= 0.0) return x >= 0.0 ? q : 31 - q;
    return x < 0.0 ? 32 + q : 63 - q;
}

PGX_EXT_HD bool ext_linear(ExtPoint& p, int which, double c)
{
    c = c + 0.0;   // -0 -> +0
    p.mode[which] = EXT_LINEAR;
    p.c[which] = c;
    return ext_finite(c);
}

PGX_EXT_HD bool ext_angular(ExtPoint& p, int which, double x, double y)
{
    if (!ext_finite(x) || !ext_finite(y) || (x == 0.0 && y == 0.0)) return false;
    p.mode[which] = EXT_ANGULAR;
    p.s[which] = ext_sector(x, y);
    return true;
}

// The coordinates of the point x in the frame row f; false: the point is not live (its label being in range is the caller's test).
PGX_EXT_HD bool ext_point(const double* f, double x0, double x1, double x2, ExtPoint& p)
{
    p.mode[0] = p.mode[1] = EXT_UNUSED;
    p.c[0] = p.c[1] = 0.0;
    p.s[0] = p.s[1] = 0;
    const double kd = f[0];
    if (!(kd == 0.0 || kd == 1.0 || kd == 2.0 || kd == 3.0 || kd == 4.0)) return false;
    if (!ext_finite(x0) || !ext_finite(x1) || !ext_finite(x2)) return false;
    const int kind = (int)kd;
    const double e[3] = {x0 - f[1], x1 - f[2], x2 - f[3]};
    const double *g = f + 4, *u = f + 7, *v = f + 10;
    switch (kind) {
    case 0: {   // plane: (e.u, e.v)
        const bool a = ext_linear(p, 0, ext_dot(e, u));
        const bool b = ext_linear(p, 1, ext_dot(e, v));
        return a && b;
    }
    case 1:   // line: e.g
        return ext_linear(p, 0, ext_dot(e, g));
    case 2: {   // cylinder, cone: (e.g, the angle about the axis)
        const bool a = ext_linear(p, 0, ext_dot(e, g));
        const bool b = ext_angular(p, 1, ext_dot(e, u), ext_dot(e, v));
        return a && b;
    }
    case 3: {   // sphere: (the cosine of the polar angle, the azimuth)
        const double ee = ext_dot(e, e);
        if (ee == 0.0) return false;
        const bool a = ext_linear(p, 0, ext_dot(e, g) / __builtin_sqrt(ee));
        const bool b = ext_angular(p, 1, ext_dot(e, u), ext_dot(e, v));
        return a && b;
    }
    default: {   // torus: (the angle about the axis, the angle about the tube's centre circle)
        const double eu = ext_dot(e, u), ev = ext_dot(e, v);
        const bool a = ext_angular(p, 0, eu, ev);
        const double rho = __builtin_sqrt(eu * eu + ev * ev);
        const bool b = ext_angular(p, 1, rho - f[13], ext_dot(e, g));
        return a && b;
    }
    }
}

PGX_EXT_HD ExtAcc ext_contribution(const ExtPoint& p)
{
    ExtAcc a;
    for (int s = 0; s < EXT_SLOTS; ++s) a.v[s] = 0;
    a.v[EXT_COUNT] = 1;
    for (int w = 0; w < 2; ++w) {
        if (p.mode[w] == EXT_LINEAR) {
            const uint64_t k = ext_key(p.c[w]);
            a.v[EXT_HI_A + 2 * w] = k;
            a.v[EXT_LO_A + 2 * w] = ~k;
        } else if (p.mode[w] == EXT_ANGULAR) {
            a.v[EXT_SEC_A + w] = (uint64_t)1 << p.s[w];
        }
    }
    return a;
}

// two contributions to the SAME instance as one
PGX_EXT_HD void ext_combine(ExtAcc& a, const ExtAcc& b)
{
    a.v[EXT_COUNT] += b.v[EXT_COUNT];
    for (int s = EXT_HI_A; s <= EXT_LO_B; ++s) a.v[s] = a.v[s] > b.v[s] ? a.v[s] : b.v[s];
    a.v[EXT_SEC_A] |= b.v[EXT_SEC_A];
    a.v[EXT_SEC_B] |= b.v[EXT_SEC_B];
}

// `Tab` gives the three updates of a table word, each ONE (atomic) operation: add(i, x), max(i, x), bor(i, x).  A zero adds nothing
// and is not sent.
template <class Tab>
PGX_EXT_HD void ext_merge(Tab& t, int64_t row, const ExtAcc& a)
{
    const int64_t base = row * EXT_SLOTS;
    if (a.v[EXT_COUNT]) t.add(base + EXT_COUNT, a.v[EXT_COUNT]);
    for (int s = EXT_HI_A; s <= EXT_LO_B; ++s)
        if (a.v[s]) t.max(base + s, a.v[s]);
    if (a.v[EXT_SEC_A]) t.bor(base + EXT_SEC_A, a.v[EXT_SEC_A]);
    if (a.v[EXT_SEC_B]) t.bor(base + EXT_SEC_B, a.v[EXT_SEC_B]);
}

// the same for one word of a table whose word i belongs to slot i % EXT_SLOTS (a workgroup's table into the global one)
template <class Tab>
PGX_EXT_HD void ext_merge_word(Tab& t, int64_t i, uint64_t x)
{
    const int s = (int)(i % EXT_SLOTS);
    if (!x) return;
    if (s == EXT_COUNT) t.add(i, x);
    else if (s <= EXT_LO_B) t.max(i, x);
    else t.bor(i, x);
}

// a finished row -> lo[2], hi[2]: an empty slot (no live point, or a coordinate that is not linear) is +inf / -inf
PGX_EXT_HD void ext_finalise(const uint64_t* row, double lo[2], double hi[2])
{
    const double inf = __builtin_inf();
    for (int w = 0; w < 2; ++w) {
        const uint64_t h = row[EXT_HI_A + 2 * w], l = row[EXT_LO_A + 2 * w];
        hi[w] = h ? ext_unkey(h) : -inf;
        lo[w] = l ? ext_unkey(~l) : inf;
    }
}

// the occupancy bin, 0..7, of one coordinate between the instance's finished bounds
PGX_EXT_HD int ext_bin(int mode, double c, int s, double lo, double hi)
{
    if (mode == EXT_ANGULAR) return s >> 3;
    if (mode != EXT_LINEAR || hi == lo) return 0;
    const double f = ((c - lo) / (hi - lo)) * 8.0;   // in [0, 8]; NaN where hi - lo overflows: bin 0
    return f >= 7.0 ? 7 : f >= 1.0 ? (int)f : 0;
}

PGX_EXT_HD uint64_t ext_occupancy_bit(const ExtPoint& p, const double lo[2], const double hi[2])
{
    const int a = ext_bin(p.mode[0], p.c[0], p.s[0], lo[0], hi[0]);
    const int b = ext_bin(p.mode[1], p.c[1], p.s[1], lo[1], hi[1]);
    return (uint64_t)1 << (8 * a + b);
}

}  // namespace pgx
