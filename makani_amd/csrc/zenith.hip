// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Cosine of the solar zenith angle (makani/third_party/climt/zenith_angle_v2.py: cos_zenith_angle), the `add_zenith` input channel:
//
//   cosz(t, phi, lambda) = sin phi sin dec + cos phi cos dec cos(theta0 + lambda),     theta0 = gmst(t) - ra(t)
//
// The reference evaluates this on the host, once per sample and once per rollout step, and uploads the plane.  Here the planes of
// all B T time levels of a call come out of ONE launch that reads the valid times from device memory, so a rollout step with a
// zenith channel stays inside a captured graph: mk_zenith_advance moves the times on behind it.
//
// Time scalars (once per block, fp64, written by one lane and broadcast through LDS; the reference holds them in fp32, where the
// days since J2000 have a grid of 1e-3 day and the sidereal-time polynomial one of 64 s = 0.27 degrees of hour angle):
//   d  = (t_us - 946 728 000 000 000) / 86 400 000 000   days since 2000-01-01T12:00 UTC, the integer difference is exact in fp64
//   jc = d / 36525;  obliquity eps, mean anomaly M, mean longitude L, equation of centre dL: the reference's polynomials
//   (x, y, z) = (cos l, cos eps sin l, sin eps sin l) with l = L + dL: the unit vector to the sun;  r = sqrt(1 - z^2)
//   dec = atan2(z, r):  sin dec = z, cos dec = r.   ra = 2 atan2(y, x + r) = atan2(y, x):  cos ra = x / r, sin ra = y / r  (x^2 + y^2 = r^2),
//   so neither angle is formed.  gmst: the polynomial is in seconds of time, reduced mod 86400 s (exact in fp64) before it becomes
//   an angle.  Every angle is reduced mod 360 degrees the same way before sincos sees it.  The first wave shares the work: three
//   of its lanes take the three independent sincos at once.
//   Kept per level, rounded once to fp32: sin dec, cos dec, cos theta0, sin theta0.
//
// Field: rank 2.  cos(theta0 + lambda) = cos theta0 cos lambda - sin theta0 sin lambda, so a pixel is three FMAs / multiplies on
// table values.  The four tables sin phi (H), cos phi (H), cos lambda (W), sin lambda (W) depend on the grid alone; mk_zenith_tables
// builds them once (fp64 sincos per entry, stored fp32), entry by entry and never incrementally, so the tables of a slice of the
// grid are the slice of the tables and an h x w shard is bit for bit the slice of the serial plane.
//
// A block owns ZROWS rows x one column segment (all W columns up to ZCOLS) of one plane.  It stages its segment of cos lambda /
// sin lambda in LDS while the first wave evaluates the scalars, then forms a[row] = sin phi sin dec and b[row] = cos phi cos dec
// for its rows.  The lanes walk the tile's groups of four consecutive pixels in row-major order (no lane idles at a row end):
//   v = fma(b, fma(-sin theta0, sin lambda, cos theta0 cos lambda), a)             five fp32 roundings behind the table values
// and write one 16-byte (f32) or 8-byte (bf16) store.  Where W % 4 != 0 or the destination is not aligned to that store the same
// kernel runs with one pixel per lane and step (P = 1): the same operations in the same order, so both paths give the same bits.
// The only traffic of plane size is the one write of the output.
#include "block_io.h"

namespace {

constexpr int ZNT = 256;
constexpr int ZROWS = 8;          // rows of a tile: 721 x 1440 gives 91 tiles of 46 KB (f32) per plane
constexpr int ZCOLS = 2048;       // columns of a segment held in LDS (2 x 8 KB)
constexpr double Z_RAD = 0.017453292519943295769;       // pi / 180

// x mod p for |x| / p < 2^20 and an integer p: k p and x - k p are exact in fp64 (a result in [0, p) up to one rounding of x / p at a
// multiple of p, which an angle does not notice)
__device__ __forceinline__ double zmod(double x, double p) { return fma(-floor(x / p), p, x); }

__device__ __forceinline__ void sincos_deg(double deg, double& s, double& c) { sincos(zmod(deg, 360.0) * Z_RAD, &s, &c); }

// sc = {sin dec, cos dec, cos theta0, sin theta0} at t_us microseconds since the Unix epoch.  Called by the whole first wave: lanes
// 0, 1, 2 take the sincos of the mean anomaly, the obliquity and GMST in the same instructions, then the ecliptic longitude, which
// needs the first of them: two fp64 sincos on the critical path instead of four.  Lane 0 writes.
__device__ void zen_time_scalars(long long t_us, float* sc) {
    const double d = (double)(t_us - 946728000000000ll) / 86400.0e6;
    const double jc = d / 36525.0;
    const double eps_deg = 23.0 + 26.0 / 60.0 + 21.406 / 3600.0 -
                           jc * (46.836769 + jc * (-0.0001831 + jc * (0.00200340 + jc * (-0.576e-6 - jc * 4.34e-8)))) / 3600.0;
    const double m_deg = 357.52910 + jc * (35999.05030 + jc * (-0.0001559 - jc * 0.00000048));
    const double l_deg = 280.46645 + jc * (36000.76983 + jc * 0.0003032);
    const double theta_s = 67310.54841 + jc * (876600.0 * 3600.0 + 8640184.812866 + jc * (0.093104 - jc * 6.2e-5));
    const int lane = threadIdx.x & 63;
    double s, c, sl, cl;
    sincos_deg(lane == 0 ? m_deg : lane == 1 ? eps_deg : zmod(theta_s, 86400.0) / 240.0, s, c);
    const double sm = __shfl(s, 0, 64), se = __shfl(s, 1, 64), ce = __shfl(c, 1, 64), sg = __shfl(s, 2, 64), cg = __shfl(c, 2, 64);
    const double cm = __shfl(c, 0, 64);
    const double s2m = 2.0 * sm * cm, s3m = sm * (3.0 - 4.0 * sm * sm);
    const double dl_deg = (1.914600 + jc * (-0.004817 - jc * 0.000014)) * sm + (0.019993 - 0.000101 * jc) * s2m + 0.000290 * s3m;
    sincos_deg(l_deg + dl_deg, sl, cl);
    const double x = cl, y = ce * sl, z = se * sl;
    const double r = sqrt(1.0 - z * z);
    const double cra = x / r, sra = y / r;              // r >= cos(obliquity) = 0.9
    if (lane == 0) {
        sc[0] = (float)z;
        sc[1] = (float)r;
        sc[2] = (float)(cg * cra + sg * sra);
        sc[3] = (float)(sg * cra - cg * sra);
    }
}

// tab = sin phi (H) | cos phi (H) | cos lambda (W) | sin lambda (W)
__global__ __launch_bounds__(ZNT) void zenith_tables_kernel(const double* __restrict__ lat_deg, const double* __restrict__ lon_deg,
                                                            float* __restrict__ tab, int H, int W) {
    const int i = blockIdx.x * ZNT + threadIdx.x;
    if (i >= H + W) return;
    double s, c;
    if (i < H) {
        sincos_deg(lat_deg[i], s, c);
        tab[i] = (float)s, tab[H + i] = (float)c;
    } else {
        const int j = i - H;
        sincos_deg(lon_deg[j], s, c);
        tab[2 * H + j] = (float)c, tab[2 * H + W + j] = (float)s;
    }
}

// grid (column segments, row tiles, B T).  cseg: columns per segment, a multiple of 4 and <= ZCOLS.  P = 4 needs W % 4 == 0 and
// every plane base aligned to four elements.
template <typename E, int P>
__global__ __launch_bounds__(ZNT) void cos_zenith_kernel(const long long* __restrict__ times, int Bt, const float* __restrict__ tab,
                                                         E* __restrict__ out, int T, int H, int W, int cseg, long long sb,
                                                         long long st) {
    __shared__ __attribute__((aligned(16))) float cl[ZCOLS];
    __shared__ __attribute__((aligned(16))) float sl[ZCOLS];
    __shared__ float ra[ZROWS], rb[ZROWS], sc[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.z / T, t = blockIdx.z - b * T;
    const int c0 = blockIdx.x * cseg, cs = min(cseg, W - c0);
    const int r0 = blockIdx.y * ZROWS, rs = min(ZROWS, H - r0);
    if (cs <= 0) return;                                    // (block-uniform)
    if (tid < 64) zen_time_scalars(times[(long long)(Bt == 1 ? 0 : b) * T + t], sc);          // (wave-uniform)
    const float* const tcl = tab + 2 * (long long)H + c0;
    for (int i = tid; i < cs; i += ZNT) cl[i] = tcl[i], sl[i] = tcl[W + i];
    __syncthreads();
    if (tid < rs) {
        ra[tid] = tab[r0 + tid] * sc[0];
        rb[tid] = tab[H + r0 + tid] * sc[1];
    }
    __syncthreads();
    const float cth = sc[2], nsth = -sc[3];
    // group q of the tile is P pixels from column P (q % qpr) of row q / qpr; a lane's next group is ZNT further on
    const int qpr = cs / P, nq = rs * qpr;
    const int dr = ZNT / qpr, dc = ZNT - dr * qpr;
    int row = tid / qpr, col = tid - row * qpr;
    E* const tile = out + ((long long)b * sb + (long long)t * st + (long long)r0 * W + c0);
    for (int q = tid; q < nq; q += ZNT) {
        const float a = ra[row], bb = rb[row];
        float v[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const int c = col * P + k;
            v[k] = fmaf(bb, fmaf(nsth, sl[c], cth * cl[c]), a);
        }
        mk_st<E, P>(tile + ((long long)row * W + col * P), v);
        col += dc, row += dr;
        if (col >= qpr) col -= qpr, ++row;
    }
}

__global__ __launch_bounds__(ZNT) void zenith_advance_kernel(long long* __restrict__ times, int n, long long dt_us) {
    for (int i = threadIdx.x; i < n; i += ZNT) times[i] += dt_us;
}

template <typename E>
void launch_cos_zenith(bool vec, dim3 grid, hipStream_t s, const long long* times, int Bt, const float* tab, void* out, int T, int H,
                       int W, int cseg, long long sb, long long st) {
    if (vec) hipLaunchKernelGGL((cos_zenith_kernel<E, 4>), grid, dim3(ZNT), 0, s, times, Bt, tab, (E*)out, T, H, W, cseg, sb, st);
    else hipLaunchKernelGGL((cos_zenith_kernel<E, 1>), grid, dim3(ZNT), 0, s, times, Bt, tab, (E*)out, T, H, W, cseg, sb, st);
}

}  // namespace

extern "C" int mk_zenith_tables(const double* lat_deg, const double* lon_deg, float* tab, int H, int W, void* stream) {
    MK_REQUIRE(lat_deg && lon_deg && tab, "zenith_tables: null pointer");
    MK_REQUIRE(H >= 1 && W >= 1 && (long long)H + W < (1ll << 30), "zenith_tables: bad grid (H %d, W %d)", H, W);
    hipLaunchKernelGGL(zenith_tables_kernel, dim3((H + W + ZNT - 1) / ZNT), dim3(ZNT), 0, (hipStream_t)stream, lat_deg, lon_deg, tab, H, W);
    return mk_check_launch("mk_zenith_tables");
}

extern "C" int mk_cos_zenith(const long long* times, int Bt, const float* tab, void* out, int dtype, int B, int T, int H, int W,
                             long long sb, long long st, void* stream) {
    MK_REQUIRE(times && tab && out, "cos_zenith: null pointer");
    MK_REQUIRE(dtype == MK_F32 || dtype == MK_BF16, "cos_zenith: dtype %d is neither f32 nor bf16", dtype);
    MK_REQUIRE(B >= 1 && T >= 1 && H >= 1 && W >= 1, "cos_zenith: bad shape (B %d, T %d, H %d, W %d)", B, T, H, W);
    MK_REQUIRE(Bt == 1 || Bt == B, "cos_zenith: times hold %d batch entries, need 1 or B = %d", Bt, B);
    MK_REQUIRE(sb >= 0 && st >= 0, "cos_zenith: negative stride (batch %lld, level %lld)", sb, st);
    MK_REQUIRE((long long)B * T <= 65535, "cos_zenith: %lld planes (B * T) exceed the grid limit of 65535", (long long)B * T);
    MK_REQUIRE(H <= 65535 * ZROWS && W <= (1 << 20), "cos_zenith: grid %d x %d exceeds the limit of %d x %d", H, W, 65535 * ZROWS, 1 << 20);
    const int nseg = (W + ZCOLS - 1) / ZCOLS;
    const int cseg = ((W + nseg - 1) / nseg + 3) / 4 * 4;            // <= ZCOLS: ZCOLS is a multiple of 4
    const size_t esz = dtype == MK_BF16 ? 2 : 4;
    const bool vec = W % 4 == 0 && sb % 4 == 0 && st % 4 == 0 && ((uintptr_t)out & (4 * esz - 1)) == 0;
    const dim3 grid(nseg, (H + ZROWS - 1) / ZROWS, B * T);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MK_BF16) launch_cos_zenith<u16>(vec, grid, s, times, Bt, tab, out, T, H, W, cseg, sb, st);
    else launch_cos_zenith<float>(vec, grid, s, times, Bt, tab, out, T, H, W, cseg, sb, st);
    return mk_check_launch("mk_cos_zenith");
}

extern "C" int mk_zenith_advance(long long* times, int n, long long dt_us, void* stream) {
    MK_REQUIRE(times && n >= 1, "zenith_advance: null pointer or n = %d", n);
    hipLaunchKernelGGL(zenith_advance_kernel, dim3(1), dim3(ZNT), 0, (hipStream_t)stream, times, n, dt_us);
    return mk_check_launch("mk_zenith_advance");
}
