// rocket_dopri5.inc — RR_INT_DOPRI5, the exact-integrator mode (SURVEY.md §8(f) rank 4).
//
// The reference's Simulator*.step (simulator.py:227-257 6DOF, :55-86 3DOF) is
// scipy.integrate.solve_ivp(method="RK45", t_span=[t, t+dt], events=ground, rtol=1e-3,
// atol=1e-6) on a float64 state. This mode runs that algorithm per env, in fp64, from
// the published scipy algorithm (pinned scipy==1.7.3, reference requirements.txt:73):
//   * common.select_initial_step (Hairer II.4; scipy >= 1.12 additionally clamps h0 to
//     the interval: RR_FLAG_SCIPY_H0_CLAMP),
//   * rk.RungeKutta._step_impl with the Dormand–Prince 5(4) tableau, RMS error norm,
//     SAFETY 0.9, factor clamp [0.2, 10], exponent -1/5, min(1, .) after a rejection,
//     min_step = 10 ulp(t),
//   * ivp.solve_ivp's event loop: a sign change of y[ev] between accepted steps
//     (find_active_events, direction 0, terminal) is located with brentq (xtol = rtol =
//     4 eps) on RkDenseOutput (quartic in theta via the P matrix) and the state becomes
//     sol(root).
// The tableau products (np.dot(K.T, a) / B / E / P in scipy, BLAS gemv / gemm, which accumulate
// with FMA on AVX2 / AVX-512 hosts) are fused multiply-adds here; the elementwise numpy
// arithmetic (the RHS, y + dy, the scalings) is not contracted.
// One lane = one env; the adaptive loop diverges per lane. The state lives in fp64
// planes (rr_env.state64); the fp32 planes are kept as its float32 cast (what the env's
// reward / bounds read, rocket_env.py:694). The clock t is not stored: the reference
// sets t = round(t + dt, 3) each step (simulator.py:245), i.e. t = round(k * dt, 3)
// after k steps of the episode, recomputed here from the counter word.
//
// The reward / done / obs epilogue restates Rocket6DOF.step / Rocket.step post-processing
// (rocket_env.py:690-719, 825-859, 986-1014, 1036-1061 / :150-247, 431-476) in the
// reference's own precision (float32 state, float64 arithmetic), not the fp32 tricks
// of the fast kernel.
//
// Included by rocket_exact.hip only, between `#pragma clang fp contract(off)` and `(fast)`, after
// rocket_device.h (which must stay outside that pragma).
#pragma once

#include "rocket_device.h"

namespace {

namespace dp {

constexpr double kG0 = 9.81, kIsp = 360.0;
constexpr double kJ[3] = {75350.25, 6037675.13, 6037675.13};
constexpr double kRT6 = -15.0;
constexpr double kI3d = 6.04e6, kSref3 = 10.5, kCd3 = 0.3, kRho3 = 1.225;
constexpr double kXcg3 = 10.0, kXcp3 = 20.0, kXt3 = 40.0;
constexpr double kPi = 3.14159265358979323846;
constexpr double kEps = 2.220446049250313e-16;

// Dormand–Prince 5(4): scipy RK45.A / B / E / P (RK45.C unused: both RHS are autonomous)
constexpr double A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
constexpr double B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
constexpr double E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
constexpr double P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};
constexpr double kSafety = 0.9, kMinFactor = 0.2, kMaxFactor = 10.0;
constexpr double kRtol = 1e-3, kAtol = 1e-6;

// Controls, fixed for one env step (simulator.py:311-318, 350-357 / :94-130).
struct XCtl {
    double tb0, tb1, tb2;  // 6DOF body-frame thrust (float32 trig products, then fp64)
    double dm;
    double delta, thrust, dom3;  // 3DOF
};

// float32 trig of a float32 argument, correctly rounded (np.cos / np.sin on float32)
__device__ __forceinline__ float cos32(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float sin32(float x) { return (float)sin((double)x); }

// _denormalize_action (rocket_env.py:969-981 / :395-406): float32 action scalar times a
// Python float is a float64 product (numpy 1.x scalar promotion), cast back to float32.
template <int MODEL>
__device__ __forceinline__ XCtl make_ctl(const XParams& X, const float* a, float* u)
{
    XCtl k{};
    if constexpr (MODEL == 6) {
        u[0] = (float)((double)a[0] * X.max_gimbal);
        u[1] = (float)((double)a[1] * X.max_gimbal);
        u[2] = (float)(((double)a[2] + 1.0) / 2.0 * X.max_thrust);
        const float cy = cos32(u[0]), sy = sin32(u[0]), cz = cos32(u[1]), sz = sin32(u[1]);
        const float p0 = cy * cz, p1 = sy * cz;
        k.tb0 = (double)p0 * (double)u[2];
        k.tb1 = (double)p1 * (double)u[2];
        k.tb2 = (double)sz * (double)u[2];
        k.dm = -(double)u[2] / (kG0 * kIsp);
    } else {
        u[0] = (float)((double)a[0] * X.max_gimbal);
        u[1] = (float)(((double)a[1] + 1.0) / 2.0 * X.max_thrust);
        const float tsd = u[1] * sin32(u[0]);
        k.delta = (double)u[0];
        k.thrust = (double)u[1];
        k.dom3 = (0.0 * (kXcg3 - kXcp3) - (double)tsd * (kXt3 - kXcg3)) / kI3d;
        k.dm = -(double)u[1] / (kIsp * kG0);
    }
    return k;
}

// 1 / x: v_rcp_f64 refined by two Newton steps (a few ulp at most, against ~10 instructions of
// a correctly rounded division): the error-norm scales of select_initial_step and the step-size
// controller, and 1 / m in the RHS.
__device__ __forceinline__ double rcp_nr(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    // v_div_fixup_f64: the IEEE special cases of 1 / x (x = +-inf -> +-0, where the Newton steps
    // give 0 * inf = NaN; 0 -> inf; NaN -> NaN), a pass-through otherwise. An inf component the
    // RHS never reads (the 3DOF altitude) then scales its error term to 0 as numpy's 1 / inf does
    return __builtin_amdgcn_div_fixup(r, x, 1.0);
}

// 1 / sqrt(x) for x > 0: v_rsq_f64 refined by two Newton steps r <- r (3 - x r^2) / 2 (a few ulp).
__device__ __forceinline__ double rsq_nr(double x)
{
    double r = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double hr = 0.5 * r;
        r = fma(hr, fma(-x * r, r, 1.0), r);
    }
    return r;
}

// Simulator6DOF.RHS (simulator.py:259-294, 297-378): DCM of q/|q| (Rotation.from_quat
// normalises), dq = 1/2 Omega(w) q with the UNnormalised q, tau = r_T x T_b.
__device__ __forceinline__ void rhs6(const XCtl& k, const double* y, double* d)
{
    const double q0 = y[6], q1 = y[7], q2 = y[8], q3 = y[9];
    // q / |q| as four products with one reciprocal square root (Rotation.from_quat divides by the
    // norm: within a few ulp per component; v_rsq_f64 + Newton instead of a correctly rounded
    // sqrt and division, ~20 VALU instructions fewer per RHS)
    const double inrm = rsq_nr(q1 * q1 + q2 * q2 + q3 * q3 + q0 * q0);
    const double x = q1 * inrm, yy = q2 * inrm, z = q3 * inrm, w = q0 * inrm;
    const double x2 = x * x, y2 = yy * yy, z2 = z * z, w2 = w * w;
    const double xy = x * yy, zw = z * w, xz = x * z, yw = yy * w, yz = yy * z, xw = x * w;
    const double R00 = x2 - y2 - z2 + w2, R01 = 2 * (xy - zw), R02 = 2 * (xz + yw);
    const double R10 = 2 * (xy + zw), R11 = -x2 + y2 - z2 + w2, R12 = 2 * (yz - xw);
    const double R20 = 2 * (xz - yw), R21 = 2 * (yz + xw), R22 = -x2 - y2 + z2 + w2;
    const double im = rcp_nr(y[13]);  // 1 / m (a few ulp)
    d[0] = y[3];
    d[1] = y[4];
    d[2] = y[5];
    d[3] = im * (R00 * k.tb0 + R01 * k.tb1 + R02 * k.tb2) - kG0;
    d[4] = im * (R10 * k.tb0 + R11 * k.tb1 + R12 * k.tb2);
    d[5] = im * (R20 * k.tb0 + R21 * k.tb1 + R22 * k.tb2);
    const double w1 = y[10], w2_ = y[11], w3 = y[12];
    d[6] = 0.5 * (-w1 * q1 - w2_ * q2 - w3 * q3);
    d[7] = 0.5 * (w1 * q0 + w3 * q2 - w2_ * q3);
    d[8] = 0.5 * (w2_ * q0 - w3 * q1 + w1 * q3);
    d[9] = 0.5 * (w3 * q0 + w2_ * q1 - w1 * q2);
    // tau = r_T x T_b with r_T = [-15, 0, 0]: np.cross's products with the zero components are
    // +-0, and adding a signed zero leaves every finite value unchanged
    const double t1 = -(kRT6 * k.tb2), t2 = kRT6 * k.tb1;
    const double j0 = kJ[0] * w1, j1 = kJ[1] * w2_, j2 = kJ[2] * w3;
    const double c0 = w2_ * j2 - w3 * j1, c1 = w3 * j0 - w1 * j2, c2 = w1 * j1 - w2_ * j0;
    d[10] = (1.0 / kJ[0]) * (-c0);
    d[11] = (1.0 / kJ[1]) * (t1 - c1);
    d[12] = (1.0 / kJ[2]) * (t2 - c2);
    d[13] = k.dm;
}

// Simulator3DOF.RHS (simulator.py:88-130): alpha = 0 so N = 0; the z drag uses cos(phi)
// (reference quirk, kept).
__device__ __forceinline__ void rhs3(const XCtl& k, const double* y, double* d)
{
    const double phi = y[2], vx = y[3], vz = y[4];
    const double Q = 0.5 * kRho3 * (vx * vx + vz * vz);
    const double Ad = kCd3 * Q * kSref3, N = 0.0 * Q * kSref3;
    const double cp = cos(phi), sp = sin(phi);
    const double ax = (k.thrust * cos(k.delta + phi) - N * sp - Ad * cp) / y[6];
    const double az = (k.thrust * sin(k.delta + phi) + N * cp - Ad * cp) / y[6] - kG0;
    d[0] = vx;
    d[1] = vz;
    d[2] = y[5];
    d[3] = ax;
    d[4] = az;
    d[5] = k.dom3;
    d[6] = k.dm;
}

template <int MODEL>
__device__ __forceinline__ void rhs(const XCtl& k, const double* y, double* d)
{
    if constexpr (MODEL == 6) rhs6(k, y, d);
    else rhs3(k, y, d);
}


// x^(-1/5) for the step-size controller (rk.py: error_norm ** error_exponent) and, through
// x^(1/5) = x (x^(-1/5))^4, select_initial_step's h1: an fp32 estimate (v_log_f32 / v_exp_f32,
// ~1e-7 relative) refined by two Newton steps on x y^5 = 1 (a few ulp), 18 VALU instructions
// against ~216 for the fp64 pow (ocml). The result only sets the next trial step size, never the
// state, so an ulp-level difference moves the state by ~1e-16 relative. Outside the fp32 estimate's
// range (and 0, inf, NaN) it is the fp64 pow.
__device__ __attribute__((noinline)) double pow_m1_5_slow(double x) { return pow(x, -1.0 / 5); }
__device__ __forceinline__ double pow_m1_5(double x)
{
    if (!(x > 1e-30 && x < 1e30)) return pow_m1_5_slow(x);
    double y = (double)__builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf((float)x));
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double y2 = y * y, y5 = y2 * y2 * y;
        y = fma(-0.2 * y, fma(x, y5, -1.0), y);
    }
    return y;
}

// common.norm: ||x|| / sqrt(n)
template <int NS>
__device__ __forceinline__ double rms_of(const double* x)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) s += x[i] * x[i];
    return sqrt(s) / sqrt((double)NS);
}

// ivp.solve_ivp(RK45, [t0, t0 + dt], y, events=y[EV] (terminal, direction 0)).
// Returns the solve_ivp status (0 reached t_bound, 1 terminal event, -1 step too small)
// and the last column of sol.y in y.
// LEAN (large N): the dense output of a terminal event runs after the step loop from the step's
// stages re-derived bit for bit, so that the loop carries no stage past its last use (256
// registers: two waves per SIMD); otherwise (one wave per SIMD anyway) it runs in the loop on the
// stages still in registers.
template <int MODEL, bool LEAN>
__device__ int solve(const XParams& X, const XCtl& c, double t0, double* y)
{
    constexpr int NS = Dims<MODEL>::NS, EV = Dims<MODEL>::EV;
    // Registers: f is the first stage K_1 (FSAL: the RHS at the accepted state), K[s - 2] holds
    // stage s = 2..7 (K[5] = the RHS at the new state), tmp holds each stage's argument and then
    // the candidate y_new. The tableau's zero coefficients (B_2 = E_2 = 0, P row 2 = 0) are
    // skipped: numpy's dot adds their 0 * K products, which leave every finite sum unchanged.
    // y_new and the error sum accumulate together, so K_3..K_6 die at y_new and the step loop's
    // peak is y, f, y_new, the error sum and K_7: with the event's dense output moved past the
    // loop the 6DOF kernel fits 256 registers, two waves per SIMD (was 360, one wave).
    double f[NS], K[6][NS], tmp[NS], ep[NS];
    const double t_bound = t0 + X.dt;
    double t = t0, t_old = t0;
    rhs<MODEL>(c, y, f);

    // select_initial_step (common.py, scipy 1.7: min(100 h0, h1); >= 1.12 clamps to the interval)
    double h_abs;
    {
        const double interval = fabs(t_bound - t);
        double sc[NS], d0s = 0.0, d1s = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            sc[i] = rcp_nr(kAtol + fabs(y[i]) * kRtol);  // 1 / scale
            const double a = y[i] * sc[i], b = f[i] * sc[i];
            d0s += a * a;
            d1s += b * b;
        }
        const double d0 = sqrt(d0s) / sqrt((double)NS), d1 = sqrt(d1s) / sqrt((double)NS);
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        if (X.clamp_h0 && h0 > interval) h0 = interval;
#pragma unroll
        for (int i = 0; i < NS; ++i) tmp[i] = y[i] + h0 * 1.0 * f[i];
        double f1[NS];
        rhs<MODEL>(c, tmp, f1);
        double d2s = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const double a = (f1[i] - f[i]) * sc[i];
            d2s += a * a;
        }
        const double d2 = sqrt(d2s) / sqrt((double)NS) / h0;
        double h1;
        if (d1 <= 1e-15 && d2 <= 1e-15) {
            h1 = fmax(1e-6, h0 * 1e-3);
        } else {  // (0.01 / max(d1, d2)) ** (1 / 5)
            const double x = 0.01 / fmax(d1, d2), r = pow_m1_5(x), r2 = r * r;
            h1 = x * (r2 * r2);
        }
        h_abs = fmin(100 * h0, h1);
        if (X.clamp_h0) {
            h_abs = fmin(h_abs, interval);
            if (interval == 0.0) h_abs = 0.0;
        }
    }

    // rk_step's stages 2..6 of a step of size h from (y, f = K_1) into K[0..4] (K_2..K_6), the
    // candidate y_new into tmp and, in the same pass, the error sum up to K_6 into ep (both
    // accumulate f, K_3..K_6 in ascending order: numpy's dot order, bitwise as two passes); the
    // same code re-derives a step's stages for the dense output (same inputs, same bits)
    auto stages = [&](double h) {
#pragma unroll
        for (int s = 1; s < 6; ++s) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                double dy = f[i] * A[s][0];  // (0 + x: numpy's dot, same value)
#pragma unroll
                for (int j = 1; j < s; ++j)
                    if (A[s][j] != 0.0) dy = fma(K[j - 1][i], A[s][j], dy);
                tmp[i] = y[i] + dy * h;
            }
            rhs<MODEL>(c, tmp, K[s - 1]);
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {  // y_new (into tmp) and the error sum without K_7
            double acc = f[i] * B[0], e = f[i] * E[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) {
                if (B[j] != 0.0) acc = fma(K[j - 1][i], B[j], acc);  // B[1] = E[1] = 0: K_2 is dead past stage 6
                if (E[j] != 0.0) e = fma(K[j - 1][i], E[j], e);
            }
            ep[i] = e;
            tmp[i] = y[i] + h * acc;
        }
    };

    auto event_out = [&]() -> int {
        // Terminal event in the step (t_old, t]: RkDenseOutput y_old + h * Q p(x), Q = K^T P,
        // p = [x, x^2, x^3, x^4], from y = y_old, f = K_1 and the step's stages in K
        const double hd = t - t_old;  // == the step's h: the same subtraction
        auto comp = [&](double tt, int i) {
            const double x = (tt - t_old) / hd;
            const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
            double q[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                double s = f[i] * P[0][cc];
#pragma unroll
                for (int j = 1; j < 7; ++j)
                    if (P[j][cc] != 0.0) s = fma(K[j - 1][i], P[j][cc], s);
                q[cc] = s;
            }
            return hd * (q[0] * p1 + q[1] * p2 + q[2] * p3 + q[3] * p4) + y[i];
        };
        // the event component's Q row once (comp() recomputes it per call; same arithmetic)
        double qev[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            double s = f[EV] * P[0][cc];
#pragma unroll
            for (int j = 1; j < 7; ++j)
                if (P[j][cc] != 0.0) s = fma(K[j - 1][EV], P[j][cc], s);
            qev[cc] = s;
        }
        const double yev = y[EV];
        auto comp_ev = [&](double tt) {
            const double x = (tt - t_old) / hd;
            const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
            return hd * (qev[0] * p1 + qev[1] * p2 + qev[2] * p3 + qev[3] * p4) + yev;
        };
        // brentq (scipy Zeros/brentq.c), xtol = rtol = 4 eps, maxiter 100
        const double xtol = 4 * kEps, rtol = 4 * kEps;
        double xpre = t_old, xcur = t, xblk = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
        double fpre = comp_ev(xpre), fcur = comp_ev(xcur);
        double root = xcur;
        if (fpre == 0) root = xpre;
        else if (fcur != 0) {
            for (int it = 0; it < 100; ++it) {
                if (fpre != 0 && fcur != 0 && (signbit(fpre) != signbit(fcur))) {
                    xblk = xpre;
                    fblk = fpre;
                    spre = scur = xcur - xpre;
                }
                if (fabs(fblk) < fabs(fcur)) {
                    xpre = xcur;
                    xcur = xblk;
                    xblk = xpre;
                    fpre = fcur;
                    fcur = fblk;
                    fblk = fpre;
                }
                const double delta = (xtol + rtol * fabs(xcur)) / 2;
                const double sbis = (xblk - xcur) / 2;
                if (fcur == 0 || fabs(sbis) < delta) break;
                if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
                    double stry;
                    if (xpre == xblk) {
                        stry = -fcur * (xcur - xpre) / (fcur - fpre);
                    } else {
                        const double dpre = (fpre - fcur) / (xpre - xcur);
                        const double dblk = (fblk - fcur) / (xblk - xcur);
                        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
                    }
                    if (2 * fabs(stry) < fmin(fabs(spre), 3 * fabs(sbis) - delta)) {
                        spre = scur;
                        scur = stry;
                    } else {
                        spre = sbis;
                        scur = sbis;
                    }
                } else {
                    spre = sbis;
                    scur = sbis;
                }
                xpre = xcur;
                fpre = fcur;
                if (fabs(scur) > delta) xcur += scur;
                else xcur += (sbis > 0 ? delta : -delta);
                fcur = comp_ev(xcur);
            }
            root = xcur;
        }
        double yr[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) yr[i] = comp(root, i);
#pragma unroll
        for (int i = 0; i < NS; ++i) y[i] = yr[i];
        return 1;
    };

    double g = y[EV], h_ev = 0.0;
    for (;;) {
        // OdeSolver.step
        bool finished = false;
        double g_new;
        if (t == t_bound) {
            t_old = t;
            finished = true;
            g_new = y[EV];
            // find_active_events on a zero-length step: sol(t) = y
            if ((g <= 0 && g_new >= 0) || (g >= 0 && g_new <= 0)) return 1;
        } else {
            // RungeKutta._step_impl (max_step = inf)
            const double min_step = 10.0 * fabs(nextafter(t, INFINITY) - t);
            if (h_abs < min_step) h_abs = min_step;
            bool rejected = false, ok = false;
            double t_new = t, h = 0.0;
            while (!ok) {
                // TOO_SMALL_STEP: status -1 (the reference's done). Written as !(h_abs >= min_step)
                // so that a NaN step size (a non-finite state or action: scipy's `h_abs < min_step`
                // is then False for ever and its step never returns) ends here too: every lane's
                // loop terminates (nonfinite() in rocket_hip.hip, the oracle's step_impl)
                if (!(h_abs >= min_step)) return -1;
                t_new = t + h_abs;
                if (t_new - t_bound > 0) t_new = t_bound;
                h = t_new - t;
                h_abs = fabs(h);
                stages(h);
                rhs<MODEL>(c, tmp, K[5]);  // K_7 = f(y_new): the next step's K_1 (FSAL)
                double es = 0.0;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const double rsc = rcp_nr(kAtol + fmax(fabs(y[i]), fabs(tmp[i])) * kRtol);
                    double e = fma(K[5][i], E[6], ep[i]);
                    e = e * h * rsc;
                    es += e * e;
                }
                const double en = sqrt(es) / sqrt((double)NS);
                if (en < 1.0) {
                    double factor = (en == 0.0) ? kMaxFactor : fmin(kMaxFactor, kSafety * pow_m1_5(en));
                    if (rejected) factor = fmin(1.0, factor);
                    h_abs *= factor;
                    ok = true;
                } else {
                    h_abs *= fmax(kMinFactor, kSafety * pow_m1_5(en));
                    rejected = true;
                }
            }
            t_old = t;
            t = t_new;
            if (t - t_bound >= 0) finished = true;
            // find_active_events: sign change of g between accepted steps, either direction (y
            // still holds y_old, f its K_1)
            g_new = tmp[EV];
            if ((g <= 0 && g_new >= 0) || (g >= 0 && g_new <= 0)) {
                if constexpr (!LEAN) return event_out();
                h_ev = h;
                break;
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) y[i] = tmp[i];
        }
        g = g_new;
        if (finished) return 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) f[i] = K[5][i];  // FSAL: the next step's K_1
    }

    if constexpr (LEAN) {
        stages(h_ev);  // the event step's stages (K_7 is still in K[5])
        return event_out();
    }
    return 0;  // not reached: the step loop returns
}

// Rotation.as_euler("zyx") of the float32 attitude quaternion (closed form).
__device__ __forceinline__ void euler_zyx(const float* q32, double* e)
{
    double w = q32[0], x = q32[1], y = q32[2], z = q32[3];
    const double nrm = sqrt(x * x + y * y + z * z + w * w);
    x /= nrm;
    y /= nrm;
    z /= nrm;
    w /= nrm;
    const double R00 = x * x - y * y - z * z + w * w;
    const double R01 = 2 * (x * y - z * w);
    double R02 = 2 * (x * z + y * w);
    const double R12 = 2 * (y * z - x * w);
    const double R22 = -x * x - y * y + z * z + w * w;
    R02 = fmin(1.0, fmax(-1.0, R02));
    e[0] = atan2(-R01, R00);
    e[1] = asin(R02);
    e[2] = atan2(-R12, R22);
}

__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

// Rocket6DOF.step post-processing on state32 = float32(state64): bounds (inclusive
// float32 Box, NaN outside), v_targ, reward terms, landing (rocket_env.py:690-719,
// 825-859, 986-1014, 1036-1061). Returns the reward (float64), fills t[5].
__device__ inline double finish6(const XParams& X, const float* s, const float* u, float v0, bool& bv, double* t)
{
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (!((double)s[i] >= X.lo[i] && (double)s[i] <= X.hi[i])) inside = false;
    bv = !inside;
    double rh0, rh1, rh2, vh0, vh1, vh2, tau;
    if ((double)s[0] > X.waypoint) {
        rh0 = (double)s[0] - X.waypoint; rh1 = s[1]; rh2 = s[2];
        vh0 = (double)s[3] + 2; vh1 = s[4]; vh2 = s[5];
        tau = 20;
    } else {
        rh0 = (double)s[0] + 1; rh1 = 0; rh2 = 0;
        vh0 = (double)s[3] + 1; vh1 = s[4]; vh2 = s[5];
        tau = 100;
    }
    const double nrh = norm3(rh0, rh1, rh2);
    const double t_go = nrh / norm3(vh0, vh1, vh2);
    const double f = -(double)v0 / fmax(1e-3, nrh) * (1 - exp(-t_go / tau));
    const double vel = X.alfa * norm3(s[3] - f * rh0, s[4] - f * rh1, s[5] - f * rh2);
    const double thr = X.beta * (double)u[2];
#if defined(RR_EXACT_INVTRIG)  // the reference's form: the zyx Euler angles by atan2 / asin
    double e[3];
    euler_zyx(&s[6], e);
    bool att = false, att_ok = false, om_ok = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (fabs(e[i]) > X.att_limit[i]) att = true;
        if (fabs(e[i]) < X.land_att_limit[i]) att_ok = true;        // any(): reference quirk
        if ((double)fabsf(s[10 + i]) < X.omega_lim[i]) om_ok = true;  // any(): reference quirk
    }
#else
    // The same tests on Rotation.as_euler("zyx") (rocket_env.py:852-855, 1040-1061) without the
    // inverse trig: a = atan2(-R01, R00) and c = atan2(-R12, R22) with |atan2(Y, X)| > L <=>
    // X < hypot(X, Y) cos L (0 <= L < pi; at X = Y = 0 atan2 is 0 or pi by the sign of X), both
    // sides homogeneous in |q|^2, so the rotation's entries stay unnormalised; b = asin(clamp(R02))
    // with |b| > L <=> |clamp(R02)| > sin L (L < pi/2), R02 normalised by ONE division (NaN -> the
    // clamp's -1, as the reference's fmin / fmax). The three fp64 atan2 / asin and three of the
    // four divisions of euler_zyx leave the finish; a test can differ from the angle comparison
    // only when the angle is within rounding of its limit.
    const double w = s[6], x = s[7], y = s[8], z = s[9];
    const double n2 = x * x + y * y + z * z + w * w;
    const double A = x * x - y * y - z * z + w * w;    // R00 |q|^2
    const double mB = -2 * (x * y - z * w);            // -R01 |q|^2
    const double D = -2 * (y * z - x * w);             // -R12 |q|^2
    const double E = -x * x - y * y + z * z + w * w;   // R22 |q|^2
    const double sb = fabs(fmin(1.0, fmax(-1.0, 2 * (x * z + y * w) / n2)));  // |sin b|
    const double ra = sqrt(A * A + mB * mB), rc = sqrt(E * E + D * D);
    // |a| > L  <=>  A < ra cos L (ra > 0); at ra = 0, |a| = pi if A is -0 (signbit), else 0
    // (limits outside [0, pi] / [0, pi/2]: the constant tests of make_xparams' bit masks)
    auto gt = [](double X_, double r_, double c_, double lim) {
        return r_ > 0.0 ? X_ < r_ * c_ : (signbit(X_) ? kPi > lim : 0.0 > lim);
    };
    auto lt = [](double X_, double r_, double c_, double lim) {
        return r_ > 0.0 ? X_ > r_ * c_ : (signbit(X_) ? kPi < lim : 0.0 < lim);
    };
    const bool att = (X.att_always != 0u) || (!(X.att_never & 1u) && gt(A, ra, X.att_c[0], X.att_limit[0])) ||
                     (!(X.att_never & 2u) && sb > X.att_c[1]) ||
                     (!(X.att_never & 4u) && gt(E, rc, X.att_c[2], X.att_limit[2]));
    const bool att_ok = (X.land_always != 0u) ||
                        (!(X.land_never & 1u) && lt(A, ra, X.land_c[0], X.land_att_limit[0])) ||
                        (!(X.land_never & 2u) && sb < X.land_c[1]) ||
                        (!(X.land_never & 4u) && lt(E, rc, X.land_c[2], X.land_att_limit[2]));  // any(): reference quirk
    bool om_ok = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if ((double)fabsf(s[10 + i]) < X.omega_lim[i]) om_ok = true;  // any(): reference quirk
#endif
    const double r = norm3(s[0], s[1], s[2]), v = norm3(s[3], s[4], s[5]);
    const bool landing = ((double)s[0] <= 1e-3) && (v < X.max_velocity) && (r < X.landing_radius) && att_ok && om_ok;
    t[0] = vel;
    t[1] = thr;
    t[2] = X.eta;
    t[3] = X.gamma * (att ? 1.0 : 0.0);
    t[4] = X.kappa * (landing ? 1.0 : 0.0);
    return t[0] + t[1] + t[2] + t[3] + t[4] + (bv ? -50.0 : 0.0);
}

// Rocket.step post-processing (3DOF), rocket_env.py:150-247, 431-476. Fills t[6].
__device__ inline double finish3(const XParams& X, const float* s, const float* u, float v0, bool& bv, double* t)
{
    bv = ((double)s[0] <= X.lo[0]) || ((double)s[0] >= X.hi[0]) || ((double)s[1] >= X.hi[1]);
    double rh0, rh1, vh0, vh1, tau;
    if ((double)s[1] > X.waypoint) {
        rh0 = s[0]; rh1 = (double)s[1] - X.waypoint;
        vh0 = s[3]; vh1 = (double)s[4] + 2;
        tau = 20;
    } else {
        rh0 = 0; rh1 = s[1];
        vh0 = s[3]; vh1 = (double)s[4] + 1;
        tau = 100;
    }
    const double nrh = sqrt(rh0 * rh0 + rh1 * rh1);
    const double t_go = nrh / sqrt(vh0 * vh0 + vh1 * vh1);
    const double f = -(double)v0 / fmax(1e-3, nrh) * (1 - exp(-t_go / tau));
    const double d0 = s[3] - f * rh0, d1 = s[4] - f * rh1;
    const double vel = X.alfa * sqrt(d0 * d0 + d1 * d1);
    const double thr = X.beta * (double)u[1];
    const double zeta = (double)s[2] - kPi / 2;
    const double r = sqrt((double)s[0] * s[0] + (double)s[1] * s[1]);
    const double v = sqrt((double)s[3] * s[3] + (double)s[4] * s[4]);
    const bool landing = ((double)s[1] <= 1e-3) && (v < X.max_velocity) && (r < X.landing_radius) &&
                         (fabs(zeta) < X.land_att_limit[0]) && ((double)fabsf(s[5]) < X.omega_lim[0]);
    t[0] = vel;
    t[1] = thr;
    t[2] = X.eta;
    t[3] = X.gamma * (fabs(zeta) > X.att_limit[0] ? 1.0 : 0.0);
    t[4] = X.delta * fmax(0.0, fabs(zeta) - kPi / 2);
    t[5] = X.kappa * (landing ? 1.0 : 0.0);
    return t[0] + t[1] + t[2] + t[3] + t[4] + t[5] + (bv ? -50.0 : 0.0);
}

}  // namespace dp

// One launch = one exact env step of all N envs (one env per lane, plain coalesced
// SoA loads/stores; this mode is about fidelity, the step is compute-bound in fp64).
// The parameters (KParams, XParams) are read through device copies where they are used: passed
// by value they were loaded into SGPRs at kernel entry and kept live across the adaptive loop,
// whose SGPR and VGPR spills then went to scratch (r03b: 69 VGPRs / 276 B per lane).
// ASOA: the action layout as a template parameter ([NA][N] planes, RR_FLAG_ACTION_SOA): as a runtime
// branch, the waitcnt pass joined the two load paths with an s_waitcnt vmcnt(0), and the [N][NA] row
// load waited for every state plane in flight — two memory round trips at the start of the step
template <int MODEL, bool LEAN, bool ASOA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(LEAN ? 2 : 1))) void step_exact_kernel(const XParams* __restrict__ xp, const Bufs B,
                                                            const StepIO io, double* state64)
{
    const KParams& P = *B.kp;
    const XParams& X = *xp;
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT;
    // diagnostic builds only (rocket_stamps.h): 0 start -> state loaded (+ make_ctl), 1 the adaptive
    // loop, 2 finish / reward / obs / terminal rows, 3 the stores issued
    RR_STAMPS_BEGIN(4);
    const int64_t n = B.n;
    const int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i0 < n;
    const int64_t i_in = valid ? i0 : n - 1;
    // every load of the step issued up front, the small ones first (one memory round trip)
    float a[NA];
    if constexpr (ASOA) {
#pragma unroll
        for (int j = 0; j < NA; ++j) a[j] = io.action[j * n + i_in];
    } else {
#pragma unroll
        for (int j = 0; j < NA; ++j) a[j] = io.action[i_in * NA + j];
    }
    float v0 = B.v0[i_in];
    uint32_t cw = B.counter[i_in];
    float ret = B.ep_ret[i_in];
    double y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state64[j * n + i_in];
    const uint32_t k_steps = cw & P.el_mask;
    // simulator clock: t_k = round(t_{k-1} + dt, 3) = rint(k * dt_milli) / 1000 (simulator.py:245)
    const double t0 = X.dt_milli > 0 ? (double)k_steps * X.dt_milli / 1000.0 : (double)k_steps * X.dt;

    float u[NA];
    const dp::XCtl c = dp::make_ctl<MODEL>(X, a, u);
    RR_STAMP_AFTER(0, y, NS);
    const int status = dp::solve<MODEL, LEAN>(X, c, t0, y);
    RR_STAMP(1);
    // the env index re-derived after the adaptive loop: otherwise the compiler keeps the 64-bit
    // addresses of the loads (14 fp64 planes, the fp32 planes, v0, counter, ...) live across the
    // loop for the stores, ~70 VGPRs that went to scratch (r03b)
    int64_t i = i_in;
    asm volatile("" : "+v"(i));
    if constexpr (MODEL == 6) {
        // _normalize_quaternion (simulator.py:250)
        const double nq = sqrt(y[6] * y[6] + y[7] * y[7] + y[8] * y[8] + y[9] * y[9]);
        y[6] /= nq;
        y[7] /= nq;
        y[8] /= nq;
        y[9] /= nq;
    } else {
        // _wrapTo2Pi (simulator.py:150-163)
        const double p2 = 2.0 * dp::kPi;
        y[2] = fmod(fmod(y[2], p2) + p2, p2);
    }
    float s[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = (float)y[j];
    bool bv;
    double td[6];
    double rd = MODEL == 6 ? dp::finish6(X, s, u, v0, bv, td) : dp::finish3(X, s, u, v0, bv, td);
    if (P.flags & RR_FLAG_REWARD_ANNEALING)  // wrappers.py:72-86
        rd = td[3] + td[NT - 1] - X.xi * ((double)a[NA - 1] + 1.0);
    const float r = (float)rd;
    bool done = status != 0 || bv;
    bool trunc = false;
    int32_t el = min((int32_t)k_steps + 1, (int32_t)P.el_mask);  // saturated as CounterLayout::time_limit
    if (P.max_steps > 0 && el >= P.max_steps) {
        trunc = !done;
        done = true;
    }
    ret += r;
    float o[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j)  // 6DOF: float32(state64 / n); 3DOF: float32(state32 / n) (rocket_env.py:963-964 / :175)
        o[j] = (float)((MODEL == 6 ? y[j] : (double)s[j]) / X.norm[j]);

    const bool dv = done && valid;
    const uint64_t m = __ballot(dv);
    if ((threadIdx.x & (kWave - 1)) == 0 && i0 < n) B.done_bits[i0 / kWave] = m;
    if (dv) {
#pragma unroll
        for (int j = 0; j < NS; ++j) B.term_obs[i * NS + j] = o[j];
        B.term_ret[i] = ret;
        B.term_len[i] = el;
        if (P.flags & RR_FLAG_AUTO_RESET) {
            const uint32_t ep = (cw >> P.ep_shift) + 1u;
            ResetStream key = reset_stream(B.kp->seed_w, P.id_off + i, cw);
            sample_ic<MODEL>(P, key, s, v0);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                y[j] = (double)s[j];
                o[j] = (float)((double)s[j] / X.norm[j]);
            }
            cw = ep << P.ep_shift;
            el = 0;
            ret = 0.0f;
        }
    }
    RR_STAMP(2);
    {
        // the obs rows [N][NS] through the wave's LDS tile as 16-B coalesced stores (store_obs_tile,
        // as the step kernel): stored from registers, each lane's row is NS dword stores 4 * NS bytes
        // apart, which took ~8 k cycles per wave to issue (tools/exact_stamps.py, r05v)
        __shared__ __attribute__((aligned(16))) float obs_lds[kBlock / kWave][kWave * NS];
        // the wave's first env as an SGPR (readfirstlane, as step_kernel): derived from the lane's i0 the
        // compiler cannot prove it uniform, and the tile's buffer stores with it as soffset become
        // waterfall loops (ADVICE r5)
        const uint32_t wave_base = blockIdx.x * kBlock + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave) * kWave;
        const uint32_t nv = (uint32_t)(n - (int64_t)wave_base);
        const uint32_t nvalid = (int64_t)wave_base >= n ? 0u : (nv < (uint32_t)kWave ? nv : (uint32_t)kWave);
        store_obs_tile<NS, kWave>(obs_lds[threadIdx.x / kWave], o, make_rsrc(io.obs, (uint64_t)NS * (uint64_t)n * 4u),
                                  wave_base, (int)(threadIdx.x & (kWave - 1)), nvalid, io.obs_vec_ok);
    }
    if (!valid) return;
    cw = (cw & ~P.el_mask) | ((uint32_t)el & P.el_mask);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        state64[j * n + i] = y[j];
        B.state[j * n + i] = (float)y[j];
    }
    B.v0[i] = v0;
    B.counter[i] = cw;
    B.ep_ret[i] = ret;
    io.reward[i] = r;
    io.done[i] = (uint8_t)done;
    if (io.truncated) io.truncated[i] = (uint8_t)trunc;
    if (io.terms) {
#pragma unroll
        for (int j = 0; j < NT; ++j) io.terms[j * n + i] = (float)td[j];
        io.terms[NT * n + i] = bv ? 1.0f : 0.0f;
        io.terms[(NT + 1) * n + i] = (float)status;  // solve_ivp status: 1 ground event, -1 failure
    }
    RR_STAMP(3);
    RR_STAMPS_WRITE(io.reward, i, (uint32_t)(threadIdx.x & (kWave - 1)), true, false);
}

}  // namespace
