/*
 * oracle/classic_control_ref.c — CPU restatement of the Gym.NET classic-control hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under gym.net_amd/ (the product) may include, link,
 * import or execute this file.  Only tests/, __graft_entry__.smoke() and the cpu_baseline leg
 * of bench.py use it, and only as the checker / the timed CPU baseline.
 *
 * PARITY UNPINNED: the reference is C# (netcoreapp3.1/net6.0); no .NET toolchain exists in
 * this image, so the reference cannot be built or run here, and its own CartPole test
 * (tests/Gym.Tests/Envs/Classic/CartpoleEnvironment.cs:14-35) asserts nothing.  This file is
 * therefore a restatement from the C# text, cross-checked bit-for-bit against an independent
 * second restatement (oracle/numpy_ref.py), against hand-derived closed forms and symmetry
 * properties (tests/test_oracle.py).  Philox4x32-10 IS pinned: it is checked against the
 * published Random123 known-answer vectors.
 * Round 3 — the closest substitute this image allows: the reference's Step() body and constant initialisers are EVALUATED
 * FROM THEIR OWN SOURCE TEXT by a small interpreter for the C# subset they use (oracle/evaluate_reference_text.py; C#'s
 * numeric promotion implemented explicitly; build container only), the resulting input -> output vectors are committed
 * (tests/golden/cartpole_reference_text.npz + its generating script), and ref_cartpole_step_f64 below reproduces all 3200 of
 * them bit for bit.  That is still not an execution of the C# (the interpreter's typing rules are the residual assumption),
 * so the header keeps saying "unpinned"; what it removes is every doubt about whether this restatement and the reference's
 * text denote the same arithmetic.
 *
 * What is restated, and from where (paths relative to /root/reference):
 *   - CartPoleEnv constants      src/Gym.Environments/Envs/Classic/CartPoleEnv.cs:24-36
 *   - CartPoleEnv.Step           src/Gym.Environments/Envs/Classic/CartPoleEnv.cs:137-186
 *   - CartPoleEnv.Reset          src/Gym.Environments/Envs/Classic/CartPoleEnv.cs:63-67
 *   - Discrete.Contains(int)     src/Gym/Spaces/Discrete.cs:38-40
 *   - Pendulum / MountainCar / Acrobot: ABSENT from the reference (README.md:69-76 lists them
 *     as unchecked roadmap items).  Restated from the upstream openai/gym classic_control
 *     algorithms as summarised in SURVEY.md Appendix B.
 * Round 4 additions (all test infrastructure like the rest):
 *   - ref_cartpole_step_f32 / numpy_ref (kernel semantics, float32 state): the INTEGER done flag is now taken from the float64 sums
 *     the reference compares (CartPoleEnv.cs:154,156,167), as the HIP kernel does — exact on every float32 input;
 *   - ref_sincos_f64_kernel, ref_cartpole_step_f64_kernel, ref_cartpole_reset_f64, ref_cartpole_autoreset_step_batch_f64: the
 *     bit-identical CPU twin of the GYMNET_FLAG_F64 kernels (the literal CartPoleEnv.cs:146-167 sequence with the kernel's own
 *     float64 sin / cos; 53-bit Philox reset draws), pinned by tests/golden/cartpole_f64_kernel.npz;
 *   - ref_acrobot_step_f32_literal: a literal float32 transcription of upstream's Acrobot formulas, the yardstick of the accuracy
 *     budget (tools/acrobot_accuracy.py, profiles/acrobot_accuracy_r04.txt) — not what any kernel runs.
 *
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off; contraction MUST stay off so that
 * the float32 "kernel semantics" functions round after every operation like the HIP kernels).
 */
#include <math.h>
#include <string.h>
#include <stdint.h>
#include <stddef.h>

/* ------------------------------------------------------------------------------------------
 * CartPole constants — CartPoleEnv.cs:24-36.  Every constant is a C# `const float`; inside
 * Step() it is widened to double.  total_mass and polemass_length are const-folded in float.
 * ---------------------------------------------------------------------------------------- */
static const float CP_GRAVITY = 9.8f;
static const float CP_MASSCART = 1.0f;
static const float CP_MASSPOLE = 0.1f;
#define CP_TOTAL_MASS ((float)(CP_MASSPOLE + CP_MASSCART))      /* 0x1.19999ap+0 */
static const float CP_LENGTH = 0.5f;
#define CP_POLEMASS_LENGTH ((float)(CP_MASSPOLE * CP_LENGTH))   /* 0x1.99999ap-5 */
static const float CP_FORCE_MAG = 10.0f;
static const float CP_TAU = 0.02f;
/* (float)(12 * 2 * Math.PI / 360) — CartPoleEnv.cs:34 */
#define CP_THETA_THRESHOLD ((float)(24.0 * 3.14159265358979323846 / 360.0))
static const float CP_X_THRESHOLD = 2.4f;

void ref_cartpole_constants(double *out10) {
    out10[0] = CP_GRAVITY;  out10[1] = CP_MASSCART;  out10[2] = CP_MASSPOLE;
    out10[3] = CP_TOTAL_MASS;  out10[4] = CP_LENGTH;  out10[5] = CP_POLEMASS_LENGTH;
    out10[6] = CP_FORCE_MAG;  out10[7] = CP_TAU;  out10[8] = CP_THETA_THRESHOLD;
    out10[9] = CP_X_THRESHOLD;
}

/* One CartPoleEnv.Step() in the reference's arithmetic (binary64 state, binary32-valued
 * constants), CartPoleEnv.cs:137-186.  state[4] = x, x_dot, theta, theta_dot (in/out);
 * *sbd = steps_beyond_done (in/out, -1 after Reset).  Returns done; *reward as the C# float.
 * Any action != 1 pushes left: validity is only Debug.Assert'ed in the reference (:139). */
int ref_cartpole_step_f64(double *state, int action, int *sbd, float *reward) {
    double x = state[0], x_dot = state[1], theta = state[2], theta_dot = state[3];
    float force = action == 1 ? CP_FORCE_MAG : -CP_FORCE_MAG;                           /* :146 */
    double costheta = cos(theta);                                                       /* :147 */
    double sintheta = sin(theta);                                                       /* :148 */
    double temp = ((double)force + (double)CP_POLEMASS_LENGTH * theta_dot * theta_dot * sintheta)
                  / (double)CP_TOTAL_MASS;                                              /* :149 */
    double thetaacc = ((double)CP_GRAVITY * sintheta - costheta * temp)
                      / ((double)CP_LENGTH * (4.0 / 3.0 - (double)CP_MASSPOLE * costheta * costheta
                                                            / (double)CP_TOTAL_MASS));  /* :150 */
    double xacc = temp - (double)CP_POLEMASS_LENGTH * thetaacc * costheta
                             / (double)CP_TOTAL_MASS;                                   /* :151 */
    /* kinematics_integrator == "euler" (:32,153): explicit Euler, OLD velocities */
    x = x + (double)CP_TAU * x_dot;                                                     /* :154 */
    x_dot = x_dot + (double)CP_TAU * xacc;                                              /* :155 */
    theta = theta + (double)CP_TAU * theta_dot;                                         /* :156 */
    theta_dot = theta_dot + (double)CP_TAU * thetaacc;                                  /* :157 */
    state[0] = x; state[1] = x_dot; state[2] = theta; state[3] = theta_dot;             /* :166 */
    int done = x < -(double)CP_X_THRESHOLD || x > (double)CP_X_THRESHOLD
            || theta < -(double)CP_THETA_THRESHOLD || theta > (double)CP_THETA_THRESHOLD; /* :167 */
    if (!done) {                                                                        /* :169 */
        *reward = 1.0f;
    } else if (*sbd == -1) {                                                            /* :171 */
        *sbd = 0;
        *reward = 1.0f;
    } else {                                                                            /* :175 */
        *sbd += 1;
        *reward = 0.0f;
    }
    return done;
}

/* The HIP kernels' sin/cos (gym.net_amd/csrc/envs.hpp: sincos_f32), restated operation for operation: 3-constant
 * Cody-Waite reduction + minimax polynomials, only IEEE mul / fma / rint => bit-identical on CPU and GPU.
 * |x| > 65536 falls back to libm here (OCML on the GPU): outside that range the two may differ by an ulp. */
void ref_sincos_f32_kernel(float x, float *s_out, float *c_out) {
    if (fabsf(x) > 65536.0f) { *s_out = sinf(x); *c_out = cosf(x); return; }
    const float n = rintf(x * 0.636619772367581343f);
    float r = fmaf(n, -1.5703125f, x);
    r = fmaf(n, -4.837512969970703125e-4f, r);
    r = fmaf(n, -7.54978995489188216e-8f, r);
    const float z = r * r;
    float ps = fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = fmaf(ps, z, -1.6666654611e-1f);
    const float s = fmaf(r * z, ps, r);
    float pc = fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = fmaf(pc, z, 4.166664568298827e-2f);
    const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
    const int q = (int)n & 3;
    const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
    *s_out = (q & 2) ? -ss : ss;
    *c_out = ((q + 1) & 2) ? -cc : cc;
}
/* The small-argument sin/cos of the Acrobot kernel (envs.hpp: sincos_small), operation for operation: two-constant
 * Cody-Waite reduction (pi/2 cut to 20 bits, so n * C1 is exact for |n| <= 15) + the same minimax polynomials with the
 * cosine in Horner form.  Acrobot's stage angles reach 33.32 rad on the env's state bounds (measured: tests/test_env_edge_tables_host.py);
 * tests/test_oracle.py holds it to 1.2e-7 of float64 over |x| <= 36.5. */
void ref_sincos_f32_small(float x, float *s_out, float *c_out) {
    const float n = rintf(x * 0.636619772367581343f);
    float r = fmaf(-0x1.921fap+0f, n, x);
    r = fmaf(-0x1.54442ep-20f, n, r);
    const float z = r * r;
    float ps = fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = fmaf(ps, z, -1.6666654611e-1f);
    const float s = fmaf(r * z, ps, r);
    float pc = fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = fmaf(pc, z, 4.166664568298827e-2f);
    pc = fmaf(pc, z, -0.5f);
    const float c = fmaf(pc, z, 1.0f);
    const int q = (int)n & 3;
    const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
    *s_out = (q & 2) ? -ss : ss;
    *c_out = ((q + 1) & 2) ? -cc : cc;
}
static inline float ksin(float x) { float s, c; ref_sincos_f32_kernel(x, &s, &c); return s; }
static inline float kcos(float x) { float s, c; ref_sincos_f32_kernel(x, &s, &c); return c; }

/* x / total_mass the way the kernel evaluates it: fma(x, zh, x*zl), zh = RN(1/C), zl = RN(1/C - zh).
 * Exposed so that tests can check it against IEEE division exhaustively. */
float ref_div_total_mass_kernel(float x) {
    const float C = CP_TOTAL_MASS;
    const float zh = 1.0f / C;
    const float zl = (float)(1.0 / (double)C - (double)zh);
    return fmaf(x, zh, x * zl);
}

/* Exhaustive check: every significand, the given biased exponents.  Returns the number of x for which
 * the kernel's constant division differs from IEEE x / total_mass. */
int64_t ref_check_div_total_mass(const int32_t *biased_exponents, int32_t count) {
    int64_t bad = 0;
    for (int32_t e = 0; e < count; ++e)
        for (uint32_t m = 0; m < (1u << 23); ++m) {
            union { uint32_t u; float f; } v;
            v.u = ((uint32_t)biased_exponents[e] << 23) | m;
            if (ref_div_total_mass_kernel(v.f) != v.f / CP_TOTAL_MASS) ++bad;
            if (ref_div_total_mass_kernel(-v.f) != -v.f / CP_TOTAL_MASS) ++bad;
        }
    return bad;
}

/* The same Step() in the HIP kernel's arithmetic: every operation in binary32 with the same
 * binary32 constants (4.0f/3.0f for the double literal), same association order, the kernel's own
 * sin/cos; the done flag from the binary64 sums the reference compares.  This is NOT the reference's arithmetic; it exists so
 * tests can require the kernel to match it BIT FOR BIT (all operations are IEEE on both sides; the
 * kernel's constant divisions are proven equal to the plain `/` written here), in addition to the
 * north_star bar of 1e-5 against ref_cartpole_step_f64. */
int ref_cartpole_step_f32(float *state, int action, int *sbd, float *reward) {
    float x = state[0], x_dot = state[1], theta = state[2], theta_dot = state[3];
    float force = action == 1 ? CP_FORCE_MAG : -CP_FORCE_MAG;
    float costheta, sintheta;
    ref_sincos_f32_kernel(theta, &sintheta, &costheta);
    float temp = (force + CP_POLEMASS_LENGTH * theta_dot * theta_dot * sintheta) / CP_TOTAL_MASS;
    float thetaacc = (CP_GRAVITY * sintheta - costheta * temp)
                     / (CP_LENGTH * (4.0f / 3.0f - CP_MASSPOLE * costheta * costheta / CP_TOTAL_MASS));
    float xacc = temp - CP_POLEMASS_LENGTH * thetaacc * costheta / CP_TOTAL_MASS;
    x = x + CP_TAU * x_dot;
    x_dot = x_dot + CP_TAU * xacc;
    theta = theta + CP_TAU * theta_dot;
    theta_dot = theta_dot + CP_TAU * thetaacc;
    /* the integer output is the reference's own: :154,156 evaluated in binary64 from the (float32-representable) inputs and
     * compared as at :167 — what the kernel does (envs.hpp CartPole::step); the stored state stays binary32 */
    double vx = (double)state[0] + (double)CP_TAU * (double)state[1];
    double vtheta = (double)state[2] + (double)CP_TAU * (double)state[3];
    state[0] = x; state[1] = x_dot; state[2] = theta; state[3] = theta_dot;
    int done = vx < -(double)CP_X_THRESHOLD || vx > (double)CP_X_THRESHOLD
            || vtheta < -(double)CP_THETA_THRESHOLD || vtheta > (double)CP_THETA_THRESHOLD;
    if (!done) { *reward = 1.0f; }
    else if (*sbd == -1) { *sbd = 0; *reward = 1.0f; }
    else { *sbd += 1; *reward = 0.0f; }
    return done;
}

/* Batched conveniences over structure-of-arrays [4][n] (the engine's HBM layout). */
void ref_cartpole_step_batch_f64(double *soa, const int32_t *action, int32_t *sbd,
                                 float *reward, uint8_t *done, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        double s[4] = { soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i] };
        int b = sbd[i];
        done[i] = (uint8_t)ref_cartpole_step_f64(s, action[i], &b, &reward[i]);
        sbd[i] = b;
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

void ref_cartpole_step_batch_f32(float *soa, const int32_t *action, int32_t *sbd,
                                 float *reward, uint8_t *done, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        float s[4] = { soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i] };
        int b = sbd[i];
        done[i] = (uint8_t)ref_cartpole_step_f32(s, action[i], &b, &reward[i]);
        sbd[i] = b;
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

/* ------------------------------------------------------------------------------------------
 * GYMNET_FLAG_F64: the engine's float64 CartPole (gym.net_amd/csrc/cartpole64.hpp), restated operation for operation.
 * It is ref_cartpole_step_f64 above — the literal CartPoleEnv.cs:141-167 sequence — with ONE substitution: Math.Sin / Math.Cos
 * (libm there) become the kernel's own sin / cos below, built from IEEE mul / add / fma / rint only, so that this function and
 * the HIP kernel agree BIT FOR BIT.  tests/test_oracle.py bounds the difference between the two sin/cos (<= 2 ulp) and hence
 * between this function and ref_cartpole_step_f64.
 * ---------------------------------------------------------------------------------------- */
/* 3-part Cody-Waite reduction (pi/2 = P1 + P2 + P3 + ..., P1 / P2 cut to 33 bits: n * P1, n * P2 exact for |n| < 2^20) and the
 * polynomial kernels published with Sun's fdlibm (k_sin.c / k_cos.c coefficients), Horner form.  |x| > 823549 -> libm. */
void ref_sincos_f64_kernel(double x, double *s_out, double *c_out) {
    if (!(fabs(x) <= 823549.0)) { *s_out = sin(x); *c_out = cos(x); return; }
    const double n = rint(x * 6.36619772367581382433e-01);
    double r = fma(-n, 1.57079632673412561417e+00, x);
    r = fma(-n, 6.07710050630396597660e-11, r);
    r = fma(-n, 2.02226624879595063154e-21, r);
    const double z = r * r;
    double ps = fma(1.58969099521155010221e-10, z, -2.50507602534068634195e-08);
    ps = fma(ps, z, 2.75573137070700676789e-06);
    ps = fma(ps, z, -1.98412698298579493134e-04);
    ps = fma(ps, z, 8.33333333332248946124e-03);
    ps = fma(ps, z, -1.66666666666666324348e-01);
    const double s = fma(r * z, ps, r);
    double pc = fma(-1.13596475577881948265e-11, z, 2.08757232129817482790e-09);
    pc = fma(pc, z, -2.75573143513906633035e-07);
    pc = fma(pc, z, 2.48015872894767294178e-05);
    pc = fma(pc, z, -1.38888888888741095749e-03);
    pc = fma(pc, z, 4.16666666666666019037e-02);
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double c = w + (((1.0 - w) - hz) + z * (z * pc));
    const int q = (int)n & 3;
    const double ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
    *s_out = (q & 2) ? -ss : ss;
    *c_out = ((q + 1) & 2) ? -cc : cc;
}

void ref_sincos_f64_kernel_batch(const double *x, double *s, double *c, int64_t n) {
    for (int64_t i = 0; i < n; ++i) ref_sincos_f64_kernel(x[i], &s[i], &c[i]);
}

/* x / total_mass the way the float64 kernel evaluates it (cartpole64.hpp DivByTotalMass64): fma(x, ZH, x * ZL) with ZH = RN(1/C),
 * ZL = RN(1/C - ZH).  tools/prove_div_total_mass_f64.py PROVES that this equals IEEE x / C for every binary64 x (C has only 24
 * significant bits: no quotient comes within 2^-24 ulp of a rounding breakpoint, the fma pair is within 2^-53 ulp of the quotient)
 * and checks the ZL literal below; ref_check_div_total_mass_f64 samples it against the hardware's division. */
double ref_div_total_mass_f64_kernel(double x) {
    const double C = (double)CP_TOTAL_MASS;
    const double ZH = 1.0 / C;
    const double ZL = -0x1.4633f3e678be9p-55;
    if (isinf(x)) return x;                  /* = x / C (C > 0); the fma pair would give inf - inf = NaN (cartpole64.hpp) */
    return fma(x, ZH, x * ZL);
}

/* `count` pseudo-random binary64 dividends (xorshift64*, both signs, exponents spread over 2^-300 .. 2^300 with most of the mass
 * in the range the step produces, plus a few special values): the number for which the fma pair differs from IEEE x / total_mass.
 * Outside the theorem, by construction (ZL < 0): x = -0 gives +0 where the division gives -0 — not observable in a step: every
 * quotient is added to / subtracted from a non-zero term (temp is (+-10 + ...) / C itself).  x = +-inf is returned as it is (the
 * division's answer; the fma pair alone would give NaN) — and is among the special values checked here. */
int64_t ref_check_div_total_mass_f64(uint64_t seed, int64_t count) {
    int64_t bad = 0;
    uint64_t s = seed ? seed : 0x9E3779B97F4A7C15ull;
    const double C = (double)CP_TOTAL_MASS;
    const double special[] = { 0.0, 1.0, -1.0, 0x1.19999ap+0, -0x1.19999ap+0, 0x1.fffffffffffffp+1000, -0x1p-900, 0x1p-900, INFINITY, -INFINITY };
    for (unsigned i = 0; i < sizeof special / sizeof special[0]; ++i) {
        const double a = ref_div_total_mass_f64_kernel(special[i]), b = special[i] / C;
        if (memcmp(&a, &b, sizeof a) != 0) ++bad;
    }
    for (int64_t i = 0; i < count; ++i) {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        const uint64_t r = s * 0x2545F4914F6CDD1Dull;
        const uint64_t mant = r & 0xFFFFFFFFFFFFFull;
        const int spread = (int)((r >> 52) & 0x3FF);                     /* 10 bits */
        const int e = (spread & 3) ? (spread >> 2) % 41 - 20 : (spread >> 2) * 600 / 256 - 300;   /* 3/4: 2^-20 .. 2^20; 1/4: 2^-300 .. 2^300 */
        union { uint64_t u; double d; } v;
        v.u = ((r >> 63) << 63) | ((uint64_t)(1023 + e) << 52) | mant;
        const double a = ref_div_total_mass_f64_kernel(v.d), b = v.d / C;
        if (a != b) ++bad;
    }
    return bad;
}

int ref_cartpole_step_f64_kernel(double *state, int action, int *sbd, float *reward) {
    double x = state[0], x_dot = state[1], theta = state[2], theta_dot = state[3];
    float force = action == 1 ? CP_FORCE_MAG : -CP_FORCE_MAG;                           /* :146 */
    double costheta, sintheta;
    ref_sincos_f64_kernel(theta, &sintheta, &costheta);                                 /* :147-148, the kernel's own */
    /* `/ total_mass` (:149-151) as the kernel evaluates it — proved equal to the plain division ref_cartpole_step_f64 keeps */
    double temp = ref_div_total_mass_f64_kernel((double)force + (double)CP_POLEMASS_LENGTH * theta_dot * theta_dot * sintheta);   /* :149 */
    double thetaacc = ((double)CP_GRAVITY * sintheta - costheta * temp)
                      / ((double)CP_LENGTH * (4.0 / 3.0 - ref_div_total_mass_f64_kernel((double)CP_MASSPOLE * costheta * costheta)));  /* :150 */
    double xacc = temp - ref_div_total_mass_f64_kernel((double)CP_POLEMASS_LENGTH * thetaacc * costheta);   /* :151 */
    x = x + (double)CP_TAU * x_dot;                                                     /* :154 */
    x_dot = x_dot + (double)CP_TAU * xacc;                                              /* :155 */
    theta = theta + (double)CP_TAU * theta_dot;                                         /* :156 */
    theta_dot = theta_dot + (double)CP_TAU * thetaacc;                                  /* :157 */
    state[0] = x; state[1] = x_dot; state[2] = theta; state[3] = theta_dot;             /* :166 */
    int done = x < -(double)CP_X_THRESHOLD || x > (double)CP_X_THRESHOLD
            || theta < -(double)CP_THETA_THRESHOLD || theta > (double)CP_THETA_THRESHOLD; /* :167 */
    if (!done) { *reward = 1.0f; }                                                      /* :168-183 */
    else if (*sbd == -1) { *sbd = 0; *reward = 1.0f; }
    else { *sbd += 1; *reward = 0.0f; }
    return done;
}

void ref_cartpole_step_batch_f64_kernel(double *soa, const int32_t *action, int32_t *sbd,
                                        float *reward, uint8_t *done, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        double s[4] = { soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i] };
        int b = sbd[i];
        done[i] = (uint8_t)ref_cartpole_step_f64_kernel(s, action[i], &b, &reward[i]);
        sbd[i] = b;
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

/* Discrete.Contains(int) — src/Gym/Spaces/Discrete.cs:38-40 (ignores Start, as the reference). */
int ref_discrete_contains(int x, int n) { return x >= 0 && x < n; }

/* ------------------------------------------------------------------------------------------
 * Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3",
 * SC'11; Random123 v1.x).  north_star replaces the reference's un-vendored NumSharp RNG
 * (CartPoleEnv.cs:49,65,196-198) with this counter-based generator; pinned by the Random123
 * known-answer vectors in tests/test_oracle.py.
 * ---------------------------------------------------------------------------------------- */
void ref_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* 24-bit uniform in [0,1): exact in binary32. */
static inline float u01_24(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

/* The engine's reset draw for global lane `lane` at engine tick `tick` with seed `seed`:
 *   counter = (lane_lo, lane_hi, tick_lo, tick_hi), key = (seed_lo, seed_hi).
 * Returns the four raw 32-bit words; each env maps them to its own reset distribution. */
void ref_reset_words(uint64_t seed, uint64_t lane, uint64_t tick, uint32_t out[4]) {
    uint32_t ctr[4] = { (uint32_t)lane, (uint32_t)(lane >> 32), (uint32_t)tick, (uint32_t)(tick >> 32) };
    uint32_t key[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
    ref_philox4x32_10(ctr, key, out);
}

/* CartPoleEnv.Reset() — CartPoleEnv.cs:63-67: sbd = -1; state ~ U(-0.05, 0.05)^4, computed as
 * low + (high-low)*u.  Kernel semantics: binary32, (high-low) = 0.1f, no contraction. */
void ref_cartpole_reset_f32(uint64_t seed, uint64_t lane, uint64_t tick, float state[4]) {
    uint32_t w[4];
    ref_reset_words(seed, lane, tick, w);
    for (int k = 0; k < 4; ++k) state[k] = -0.05f + 0.1f * u01_24(w[k]);
}

void ref_cartpole_reset_batch_f32(uint64_t seed, uint64_t lane0, uint64_t tick, float *soa, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        float s[4];
        ref_cartpole_reset_f32(seed, lane0 + (uint64_t)i, tick, s);
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

/* GYMNET_FLAG_F64 reset draw (cartpole64.hpp CartPole64::reset): CartPoleEnv.cs:63-67 in float64, low + (high - low) * u
 * with u a 53-bit uniform ((a >> 5) * 2^26 + (b >> 6)) / 2^53 — NumPy's random_sample() construction — where a is word k of
 * the float32 engine's Philox call (key = seed) and b is word k of a second call with key ^ 0xC2B2AE3D27D4EB4F. */
#define REF_RESET64_STREAM 0xC2B2AE3D27D4EB4Full
void ref_cartpole_reset_f64(uint64_t seed, uint64_t lane, uint64_t tick, double state[4]) {
    uint32_t a[4], b[4];
    ref_reset_words(seed, lane, tick, a);
    ref_reset_words(seed ^ REF_RESET64_STREAM, lane, tick, b);
    for (int k = 0; k < 4; ++k) {
        double u = ((double)(a[k] >> 5) * 67108864.0 + (double)(b[k] >> 6)) * (1.0 / 9007199254740992.0);
        state[k] = -0.05 + (0.05 - -0.05) * u;
    }
}

void ref_cartpole_reset_batch_f64(uint64_t seed, const uint64_t *lane_seed, uint64_t lane0, uint64_t tick, double *soa, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        double s[4];
        ref_cartpole_reset_f64(lane_seed ? lane_seed[i] : seed, lane0 + (uint64_t)i, tick, s);
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

/* One vector step of a GYMNET_FLAG_F64 handle with the fused auto-reset (the float64 twin of ref_env_autoreset_step_batch_f32). */
void ref_cartpole_autoreset_step_batch_f64(uint64_t seed, const uint64_t *lane_seed, uint64_t lane0, uint64_t tick,
                                           double *soa, const int32_t *action, float *reward, uint8_t *done, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        double s[4] = { soa[i], soa[n + i], soa[2 * n + i], soa[3 * n + i] };
        int b = -1;
        const int d = ref_cartpole_step_f64_kernel(s, action[i], &b, &reward[i]);
        if (d) ref_cartpole_reset_f64(lane_seed ? lane_seed[i] : seed, lane0 + (uint64_t)i, tick, s);
        done[i] = (uint8_t)d;
        soa[i] = s[0]; soa[n + i] = s[1]; soa[2 * n + i] = s[2]; soa[3 * n + i] = s[3];
    }
}

/* Space sampling draws from the engine's ACTION stream, version 2 (csrc/philox.hpp): a sampled action consumes ONE 32-bit word
 * and a Philox4x32-10 call yields four, so the four consecutive global lanes of a group share a call:
 *     word A of global lane L at tick t = word (L & 3) of Philox(key = seed ^ 0x9E3779B97F4A7C15, counter = (L >> 2, t))
 *     word B of global lane L at tick t = word (L & 3) of Philox(key = seed ^ 0xD6E8FEB86659FD93, counter = (L >> 2, t))
 * A is the ActionSpace.Sample() word; B is the second word of the consumers that need one (the epsilon-greedy coin, the second
 * uniform of Box.cs:82's normal).  The keys differ from the reset draws' (key = seed), so ActionSpace.Sample() with an env's own
 * (seed, tick) can never replay the words of that env's reset draw.  (Version 1 made a whole call per lane, counter (L, t), and
 * used its words 0 and 1.)  Written lane by lane on purpose — the kernels share the call per thread; the oracle recomputes it. */
#define REF_ACTION_STREAM 0x9E3779B97F4A7C15ull
#define REF_AUX_STREAM 0xD6E8FEB86659FD93ull
uint32_t ref_action_word(uint64_t seed, uint64_t lane, uint64_t tick) {
    uint32_t w[4];
    ref_reset_words(seed ^ REF_ACTION_STREAM, lane >> 2, tick, w);
    return w[lane & 3u];
}
uint32_t ref_aux_word(uint64_t seed, uint64_t lane, uint64_t tick) {
    uint32_t w[4];
    ref_reset_words(seed ^ REF_AUX_STREAM, lane >> 2, tick, w);
    return w[lane & 3u];
}
/* both words of `count` consecutive lanes (tests cross-check them against the NumPy Philox twin) */
void ref_action_words_batch(uint64_t seed, uint64_t lane0, uint64_t tick, uint32_t *word_a, uint32_t *word_b, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        word_a[i] = ref_action_word(seed, lane0 + (uint64_t)i, tick);
        word_b[i] = ref_aux_word(seed, lane0 + (uint64_t)i, tick);
    }
}

/* Discrete.Sample() — src/Gym/Spaces/Discrete.cs:17-28 (no mask): Start + randint(0, N).
 * Engine semantics: value = start + hi32(word A * n) (Lemire multiply-shift; exact-uniform when n is a power of two). */
int32_t ref_discrete_sample(uint64_t seed, uint64_t lane, uint64_t tick, int32_t n, int32_t start) {
    return start + (int32_t)(((uint64_t)ref_action_word(seed, lane, tick) * (uint64_t)(uint32_t)n) >> 32);
}

/* Discrete.Sample(mask) — Discrete.cs:18-26: bmask = (mask == 1); any -> Start + choice(nonzero(bmask)); none -> Start.
 * Engine semantics: choice(k) = hi32(word A * k) with the word the unmasked draw uses.  mask: one row of n bytes per lane
 * (mask_stride = n) or one shared row (mask_stride = 0). */
void ref_discrete_sample_masked_batch(uint64_t seed, uint64_t lane0, uint64_t tick, int32_t n, int32_t start,
                                      const uint8_t *mask, int64_t mask_stride, int32_t *out, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t *m = mask + i * mask_stride;
        int32_t valid = 0, pick = 0;
        for (int32_t k = 0; k < n; ++k) valid += m[k] == 1;
        if (valid > 0) {
            const uint32_t wa = ref_action_word(seed, lane0 + (uint64_t)i, tick);
            int32_t want = (int32_t)(((uint64_t)wa * (uint64_t)(uint32_t)valid) >> 32);
            for (int32_t k = 0; k < n; ++k)
                if (m[k] == 1) { if (want == 0) { pick = k; break; } --want; }
        }
        out[i] = start + pick;
    }
}

void ref_discrete_sample_batch(uint64_t seed, uint64_t lane0, uint64_t tick, int32_t n, int32_t start,
                               int32_t *out, int64_t count) {
    for (int64_t i = 0; i < count; ++i) out[i] = ref_discrete_sample(seed, lane0 + (uint64_t)i, tick, n, start);
}

/* The engine's batched epsilon-greedy composer (TrainingPlaySession.cs:46-52): explore iff u01_24(word B) <= epsilon; the explored
 * action is the Discrete.Sample() draw (word A) of the same (seed, lane, tick). */
void ref_compose_discrete_batch(uint64_t seed, uint64_t lane0, uint64_t tick, int32_t n, float epsilon,
                                const int32_t *policy, int32_t *out, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        const uint64_t lane = lane0 + (uint64_t)i;
        out[i] = u01_24(ref_aux_word(seed, lane, tick)) <= epsilon ? ref_discrete_sample(seed, lane, tick, n, 0) : policy[i];
    }
}

/* Box.Sample() bounded regime — src/Gym/Spaces/Box.cs:69-90: uniform(low, high). Engine
 * semantics (binary32): low + (high-low)*u with u = 24-bit uniform from word A; where high-low overflows binary32 (bounds as wide as
 * CartPole's +-float.MaxValue velocity components) the convex form low*(1-u) + high*u, which cannot overflow (csrc/kernels.hip
 * box_sample_value). */
void ref_box_uniform_sample_batch(uint64_t seed, uint64_t lane0, uint64_t tick, float low, float high,
                                  float *out, int64_t count) {
    const float width = high - low;
    for (int64_t i = 0; i < count; ++i) {
        const float u = u01_24(ref_action_word(seed, lane0 + (uint64_t)i, tick));
        out[i] = isfinite(width) ? low + width * u : low * (1.0f - u) + high * u;
    }
}

/* ------------------------------------------------------------------------------------------
 * Envs that are NOT in the reference (README.md:69-76): upstream openai/gym classic_control,
 * SURVEY.md Appendix B.  f64 = "upstream semantics", f32 = "kernel semantics".
 * ---------------------------------------------------------------------------------------- */
#define PI_D 3.14159265358979323846
#define PI_F 3.14159265358979323846f

/* Pendulum-v1.  state = (theta, theta_dot); obs = (cos th', sin th', thdot'); never terminates. */
static inline double floored_mod_d(double a, double m) { double r = fmod(a, m); if (r < 0.0) r += m; return r; }
static inline float floored_mod_f(float a, float m) { float r = fmodf(a, m); if (r < 0.0f) r += m; return r; }

/* The Pendulum kernel's fmodf(a, 2 pi) (envs.hpp Pendulum::fmod_2pi), restated: truncated quotient from one multiply, exact
 * remainder by fma, one repair step.  It is EXACT — identical to libm's fmodf for every finite |a| < 2^22 * 2 pi — which is why
 * ref_pendulum_step_f32 below may keep calling fmodf; ref_check_fmod_2pi counts the arguments for which that fails. */
float ref_fmod_2pi_kernel(float a) {
    const float m = 2.0f * PI_F, inv_m = 1.0f / m;
    const float ax = fabsf(a);
    if (!(ax < 4194304.0f * m)) return fmodf(a, m);
    float q = truncf(ax * inv_m);
    float r = fmaf(-q, m, ax);
    q = r < 0.0f ? q - 1.0f : (r >= m ? q + 1.0f : q);
    r = fmaf(-q, m, ax);
    return copysignf(r, a);
}

/* every `stride`-th binary32 bit pattern below 2^22 * 2 pi (both signs), and the 7 floats around each of the first `multiples`
 * multiples of 2 pi — the arguments where a quotient off by one would show */
int64_t ref_check_fmod_2pi(uint32_t stride, int32_t multiples) {
    const float m = 2.0f * PI_F;
    int64_t bad = 0;
    for (uint64_t bits = 0; bits < 0x4c000000ull; bits += stride) {
        const uint32_t b = (uint32_t)bits;
        float a;
        memcpy(&a, &b, 4);
        for (int sgn = 0; sgn < 2; ++sgn) {
            const float x = sgn ? -a : a, w = fmodf(x, m), g = ref_fmod_2pi_kernel(x);
            if (memcmp(&w, &g, 4) != 0) ++bad;
        }
    }
    for (int32_t k = 1; k <= multiples; ++k) {
        const float f = (float)((double)k * (double)m);
        for (int d = -3; d <= 3; ++d) {
            float a = f;
            for (int t = 0; t < (d < 0 ? -d : d); ++t) a = nextafterf(a, d < 0 ? 0.0f : INFINITY);
            const float w = fmodf(a, m), g = ref_fmod_2pi_kernel(a);
            if (memcmp(&w, &g, 4) != 0) ++bad;
        }
    }
    return bad;
}

void ref_pendulum_step_f64(double *state, double a, double *obs3, double *reward) {
    const double g = 10.0, m = 1.0, l = 1.0, dt = 0.05, max_speed = 8.0, max_torque = 2.0;
    double th = state[0], thdot = state[1];
    double u = a < -max_torque ? -max_torque : (a > max_torque ? max_torque : a);
    double nrm = floored_mod_d(th + PI_D, 2.0 * PI_D) - PI_D;
    double costs = nrm * nrm + 0.1 * (thdot * thdot) + 0.001 * (u * u);
    double newthdot = thdot + (3.0 * g / (2.0 * l) * sin(th) + 3.0 / (m * (l * l)) * u) * dt;
    newthdot = newthdot < -max_speed ? -max_speed : (newthdot > max_speed ? max_speed : newthdot);
    double newth = th + newthdot * dt;
    state[0] = newth; state[1] = newthdot;
    obs3[0] = cos(newth); obs3[1] = sin(newth); obs3[2] = newthdot;
    *reward = -costs;
}

void ref_pendulum_step_f32(float *state, float a, float *obs3, float *reward) {
    const float max_speed = 8.0f, max_torque = 2.0f, dt = 0.05f;
    float th = state[0], thdot = state[1];
    float u = a < -max_torque ? -max_torque : (a > max_torque ? max_torque : a);
    float nrm = floored_mod_f(th + PI_F, 2.0f * PI_F) - PI_F;
    float costs = nrm * nrm + 0.1f * (thdot * thdot) + 0.001f * (u * u);
    float newthdot = thdot + (15.0f * ksin(th) + 3.0f * u) * dt;   /* 3g/(2l) = 15, 3/(m l^2) = 3 */
    newthdot = newthdot < -max_speed ? -max_speed : (newthdot > max_speed ? max_speed : newthdot);
    float newth = th + newthdot * dt;
    state[0] = newth; state[1] = newthdot;
    ref_sincos_f32_kernel(newth, &obs3[1], &obs3[0]); obs3[2] = newthdot;
    *reward = -costs;
}

void ref_pendulum_reset_f32(uint64_t seed, uint64_t lane, uint64_t tick, float state[2]) {
    uint32_t w[4];
    ref_reset_words(seed, lane, tick, w);
    state[0] = -PI_F + (2.0f * PI_F) * u01_24(w[0]);
    state[1] = -1.0f + 2.0f * u01_24(w[1]);
}

/* MountainCar-v0.  state = (position, velocity); a in {0,1,2}. */
int ref_mountaincar_step_f64(double *state, int a, double *reward) {
    double p = state[0], v = state[1];
    v += (a - 1) * 0.001 + cos(3.0 * p) * (-0.0025);
    v = v < -0.07 ? -0.07 : (v > 0.07 ? 0.07 : v);
    p += v;
    p = p < -1.2 ? -1.2 : (p > 0.6 ? 0.6 : p);
    if (p == -1.2 && v < 0.0) v = 0.0;
    state[0] = p; state[1] = v;
    *reward = -1.0;
    return p >= 0.5 && v >= 0.0;
}

int ref_mountaincar_step_f32(float *state, int a, float *reward) {
    float p = state[0], v = state[1];
    v += (float)(a - 1) * 0.001f + kcos(3.0f * p) * (-0.0025f);
    v = v < -0.07f ? -0.07f : (v > 0.07f ? 0.07f : v);
    p += v;
    p = p < -1.2f ? -1.2f : (p > 0.6f ? 0.6f : p);
    if (p == -1.2f && v < 0.0f) v = 0.0f;
    state[0] = p; state[1] = v;
    *reward = -1.0f;
    return p >= 0.5f && v >= 0.0f;
}

void ref_mountaincar_reset_f32(uint64_t seed, uint64_t lane, uint64_t tick, float state[2]) {
    uint32_t w[4];
    ref_reset_words(seed, lane, tick, w);
    state[0] = -0.6f + 0.2f * u01_24(w[0]);
    state[1] = 0.0f;
}

/* Acrobot-v1 ("book" dynamics, RK4, dt = 0.2).  state = (th1, th2, dth1, dth2); a in {0,1,2}. */
static void acrobot_dsdt_f64(const double s[4], double tau, double d[4]) {
    const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
    double th1 = s[0], th2 = s[1], dth1 = s[2], dth2 = s[3];
    double d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * cos(th2)) + I1 + I2;
    double d2 = m2 * (lc2 * lc2 + l1 * lc2 * cos(th2)) + I2;
    double phi2 = m2 * lc2 * g * cos(th1 + th2 - PI_D / 2.0);
    double phi1 = -m2 * l1 * lc2 * dth2 * dth2 * sin(th2)
                  - 2.0 * m2 * l1 * lc2 * dth2 * dth1 * sin(th2)
                  + (m1 * lc1 + m2 * l1) * g * cos(th1 - PI_D / 2.0) + phi2;
    double ddth2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * dth1 * dth1 * sin(th2) - phi2)
                   / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1);
    double ddth1 = -(d2 * ddth2 + phi1) / d1;
    d[0] = dth1; d[1] = dth2; d[2] = ddth1; d[3] = ddth2;
}

/* upstream's loops, unbounded.  (An infinite angle would never leave them — upstream hangs there — so it is handed back as it came;
 * no test reads that as upstream's answer.)  count: how many times the body ran. */
static double wrap_d_count(double x, double m, double M, int *count) {
    double diff = M - m;
    int c = 0;
    if (isinf(x)) { if (count) *count = -1; return x; }
    while (x > M) { x -= diff; ++c; }
    while (x < m) { x += diff; ++c; }
    if (count) *count = c;
    return x;
}
static double wrap_d(double x, double m, double M) { return wrap_d_count(x, m, M, 0); }

static int acrobot_step_f64_probe(double *state, int a, double *obs6, double *reward, int *wraps2, double *probe3) {
    const double dt = 0.2, mv1 = 4.0 * PI_D, mv2 = 9.0 * PI_D;
    double tau = (double)(a - 1);
    double k1[4], k2[4], k3[4], k4[4], y[4], big = fmax(fabs(state[0]), fabs(state[1]));
    int w[2];
    acrobot_dsdt_f64(state, tau, k1);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 2.0 * k1[i];
    big = fmax(big, fmax(fabs(y[0]), fabs(y[1])));
    acrobot_dsdt_f64(y, tau, k2);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 2.0 * k2[i];
    big = fmax(big, fmax(fabs(y[0]), fabs(y[1])));
    acrobot_dsdt_f64(y, tau, k3);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt * k3[i];
    big = fmax(big, fmax(fabs(y[0]), fabs(y[1])));
    acrobot_dsdt_f64(y, tau, k4);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    if (probe3) { probe3[0] = y[0]; probe3[1] = y[1]; probe3[2] = big; }
    y[0] = wrap_d_count(y[0], -PI_D, PI_D, &w[0]);
    y[1] = wrap_d_count(y[1], -PI_D, PI_D, &w[1]);
    if (wraps2) { wraps2[0] = w[0]; wraps2[1] = w[1]; }
    y[2] = y[2] < -mv1 ? -mv1 : (y[2] > mv1 ? mv1 : y[2]);
    y[3] = y[3] < -mv2 ? -mv2 : (y[3] > mv2 ? mv2 : y[3]);
    for (int i = 0; i < 4; ++i) state[i] = y[i];
    int done = (-cos(y[0]) - cos(y[1] + y[0])) > 1.0;
    *reward = done ? 0.0 : -1.0;
    obs6[0] = cos(y[0]); obs6[1] = sin(y[0]); obs6[2] = cos(y[1]); obs6[3] = sin(y[1]);
    obs6[4] = y[2]; obs6[5] = y[3];
    return done;
}

int ref_acrobot_step_f64(double *state, int a, double *obs6, double *reward) {
    return acrobot_step_f64_probe(state, a, obs6, reward, 0, 0);
}

/* 1/P for P = d1 * det in [6.4, 11.6] (kernel semantics, gym.net_amd/csrc/envs.hpp Acrobot::recip_p): quadratic minimax
 * seed + two Newton steps, fma only. */
static float acrobot_recip_p_f32(float P) {
    float r = fmaf(fmaf(P, 0x1.82ab8p-10f, -0x1.4640b2p-5f), P, 0x1.6677a2p-2f);
    r = fmaf(r, fmaf(-P, r, 1.0f), r);
    r = fmaf(r, fmaf(-P, r, 1.0f), r);
    return r;
}

static void acrobot_dsdt_f32(const float s[4], float tau, float d[4]) {
    /* kernel semantics (gym.net_amd/csrc/envs.hpp Acrobot::dsdt), operation for operation: constants folded (m1=m2=l1=I1=I2=1,
     * lc1=lc2=0.5, g=9.8); cos(th1+th2-pi/2) = sin(th1+th2) = s1*c2 + c1*s2, cos(th1-pi/2) = s1; numerator and denominator of
     * ddth2 multiplied through by d1 so that ONE reciprocal R = 1/(d1*det) serves both accelerations; every a*b+c is an fmaf */
    float th1 = s[0], th2 = s[1], A = s[2], B = s[3];
    float s1, c1, s2, c2;
    ref_sincos_f32_small(th1, &s1, &c1);
    ref_sincos_f32_small(th2, &s2, &c2);
    float d1 = c2 + 3.5f;
    float d2 = fmaf(0.5f, c2, 1.25f);
    float phi2 = 4.9f * fmaf(s1, c2, c1 * s2);
    float phi1 = fmaf(-(s2 * B), fmaf(0.5f, B, A), fmaf(14.7f, s1, phi2));
    float h = fmaf(-(0.5f * A), A * s2, tau - phi2);
    float det = fmaf(1.25f, d1, -(d2 * d2));
    float num = fmaf(h, d1, d2 * phi1);
    float R = acrobot_recip_p_f32(d1 * det);
    float ddth2 = num * (R * d1);
    float ddth1 = -fmaf(d2, ddth2, phi1) * (R * det);
    d[0] = A; d[1] = B; d[2] = ddth1; d[3] = ddth2;
}

/* kernel semantics (envs.hpp Acrobot::wrap): upstream's `while x > M: x -= diff` / `while x < m: x += diff` with m = -M, as a
 * BOUNDED chain on the magnitude — at most k subtractions, then the sign bit of the input put back by xor.  Only one of the two
 * upstream loops can ever run and x + diff == -(|x| - diff) bit for bit, so whenever k subtractions suffice (|x| <= (2k + 1) M)
 * this is upstream's result; beyond that — and for +-inf / NaN, where upstream's loop never ends — the angle keeps what is left
 * after k subtractions.  ACROBOT_WRAP_K is the kernel's k: the measured pre-wrap maximum over the closed state box, 29.73 rad,
 * plus one full turn needs (2k + 1) pi >= 36.01, i.e. k = 6 (tests/test_env_edge_tables_host.py measures it again). */
#define ACROBOT_WRAP_K 6
static float wrap_f_k(float x, float M, int k, int *count) {
    const float diff = M + M;
    uint32_t bits, sign;
    float ax = fabsf(x);
    int c = 0;
    memcpy(&bits, &x, 4);
    sign = bits & 0x80000000u;
    for (int i = 0; i < k && ax > M; ++i) { ax -= diff; ++c; }
    if (count) *count = c;
    memcpy(&bits, &ax, 4);
    bits ^= sign;
    memcpy(&ax, &bits, 4);
    return ax;
}
static float wrap_f(float x, float m, float M) { (void)m; return wrap_f_k(x, M, ACROBOT_WRAP_K, 0); }

/* probe (optional, may be null): [0..1] the angles before the wrap, [2] the largest |angle| handed to sin / cos by the four stages */
static int acrobot_step_f32_k(float *state, int a, float *obs6, float *reward, int k, int *wraps2, float *probe3) {
    const float dt = 0.2f, mv1 = 4.0f * PI_F, mv2 = 9.0f * PI_F;
    float tau = (float)(a - 1);
    float k1[4], k2[4], k3[4], k4[4], y[4], big = fmaxf(fabsf(state[0]), fabsf(state[1]));
    int w[2];
    acrobot_dsdt_f32(state, tau, k1);
    for (int i = 0; i < 4; ++i) y[i] = fmaf(dt / 2.0f, k1[i], state[i]);
    big = fmaxf(big, fmaxf(fabsf(y[0]), fabsf(y[1])));
    acrobot_dsdt_f32(y, tau, k2);
    for (int i = 0; i < 4; ++i) y[i] = fmaf(dt / 2.0f, k2[i], state[i]);
    big = fmaxf(big, fmaxf(fabsf(y[0]), fabsf(y[1])));
    acrobot_dsdt_f32(y, tau, k3);
    for (int i = 0; i < 4; ++i) y[i] = fmaf(dt, k3[i], state[i]);
    big = fmaxf(big, fmaxf(fabsf(y[0]), fabsf(y[1])));
    acrobot_dsdt_f32(y, tau, k4);
    for (int i = 0; i < 4; ++i) y[i] = fmaf(dt / 6.0f, fmaf(2.0f, k3[i], fmaf(2.0f, k2[i], k1[i])) + k4[i], state[i]);
    if (probe3) { probe3[0] = y[0]; probe3[1] = y[1]; probe3[2] = big; }
    y[0] = wrap_f_k(y[0], PI_F, k, &w[0]);
    y[1] = wrap_f_k(y[1], PI_F, k, &w[1]);
    if (wraps2) { wraps2[0] = w[0]; wraps2[1] = w[1]; }
    y[2] = y[2] < -mv1 ? -mv1 : (y[2] > mv1 ? mv1 : y[2]);
    y[3] = y[3] < -mv2 ? -mv2 : (y[3] > mv2 ? mv2 : y[3]);
    for (int i = 0; i < 4; ++i) state[i] = y[i];
    ref_sincos_f32_small(y[0], &obs6[1], &obs6[0]); ref_sincos_f32_small(y[1], &obs6[3], &obs6[2]);
    int done = (-obs6[0] - fmaf(obs6[0], obs6[2], -(obs6[1] * obs6[3]))) > 1.0f;
    *reward = done ? 0.0f : -1.0f;
    obs6[4] = y[2]; obs6[5] = y[3];
    return done;
}

int ref_acrobot_step_f32(float *state, int a, float *obs6, float *reward) {
    return acrobot_step_f32_k(state, a, obs6, reward, ACROBOT_WRAP_K, 0, 0);
}

int ref_acrobot_wrap_k(void) { return ACROBOT_WRAP_K; }

/* A LITERAL binary32 transcription of upstream's dsdt / rk4 (the float64 code above with every double replaced by float, libm
 * sinf / cosf, IEEE division, upstream's association order) — NOT what the kernel runs.  It exists for one purpose: the accuracy
 * budget of tools/acrobot_accuracy.py, which compares the error of THIS against the float64 restatement with the
 * error of the shipped instruction-diet form (acrobot_dsdt_f32 above), to show how much of the float32-vs-float64 difference is
 * RK4 amplifying float32 rounding and how much the diet adds. */
static void acrobot_dsdt_f32_literal(const float s[4], float tau, float d[4]) {
    const float m1 = 1.0f, m2 = 1.0f, l1 = 1.0f, lc1 = 0.5f, lc2 = 0.5f, I1 = 1.0f, I2 = 1.0f, g = 9.8f;
    float th1 = s[0], th2 = s[1], dth1 = s[2], dth2 = s[3];
    float d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0f * l1 * lc2 * cosf(th2)) + I1 + I2;
    float d2 = m2 * (lc2 * lc2 + l1 * lc2 * cosf(th2)) + I2;
    float phi2 = m2 * lc2 * g * cosf(th1 + th2 - PI_F / 2.0f);
    float phi1 = -m2 * l1 * lc2 * dth2 * dth2 * sinf(th2)
                 - 2.0f * m2 * l1 * lc2 * dth2 * dth1 * sinf(th2)
                 + (m1 * lc1 + m2 * l1) * g * cosf(th1 - PI_F / 2.0f) + phi2;
    float ddth2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * dth1 * dth1 * sinf(th2) - phi2)
                  / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1);
    float ddth1 = -(d2 * ddth2 + phi1) / d1;
    d[0] = dth1; d[1] = dth2; d[2] = ddth1; d[3] = ddth2;
}

int ref_acrobot_step_f32_literal(float *state, int a, float *obs6, float *reward) {
    const float dt = 0.2f, mv1 = 4.0f * PI_F, mv2 = 9.0f * PI_F;
    float tau = (float)(a - 1);
    float k1[4], k2[4], k3[4], k4[4], y[4];
    acrobot_dsdt_f32_literal(state, tau, k1);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 2.0f * k1[i];
    acrobot_dsdt_f32_literal(y, tau, k2);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 2.0f * k2[i];
    acrobot_dsdt_f32_literal(y, tau, k3);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt * k3[i];
    acrobot_dsdt_f32_literal(y, tau, k4);
    for (int i = 0; i < 4; ++i) y[i] = state[i] + dt / 6.0f * (k1[i] + 2.0f * k2[i] + 2.0f * k3[i] + k4[i]);
    y[0] = wrap_f(y[0], -PI_F, PI_F);
    y[1] = wrap_f(y[1], -PI_F, PI_F);
    y[2] = y[2] < -mv1 ? -mv1 : (y[2] > mv1 ? mv1 : y[2]);
    y[3] = y[3] < -mv2 ? -mv2 : (y[3] > mv2 ? mv2 : y[3]);
    for (int i = 0; i < 4; ++i) state[i] = y[i];
    int done = (-cosf(y[0]) - cosf(y[1] + y[0])) > 1.0f;
    *reward = done ? 0.0f : -1.0f;
    obs6[0] = cosf(y[0]); obs6[1] = sinf(y[0]); obs6[2] = cosf(y[1]); obs6[3] = sinf(y[1]);
    obs6[4] = y[2]; obs6[5] = y[3];
    return done;
}

void ref_acrobot_step_batch_f32_literal(float *state_soa, const int32_t *action, float *obs_soa, float *reward, uint8_t *done, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        float s[4], o[6], r;
        for (int k = 0; k < 4; ++k) s[k] = state_soa[(int64_t)k * n + i];
        done[i] = (uint8_t)ref_acrobot_step_f32_literal(s, action[i], o, &r);
        reward[i] = r;
        for (int k = 0; k < 4; ++k) state_soa[(int64_t)k * n + i] = s[k];
        for (int k = 0; k < 6; ++k) obs_soa[(int64_t)k * n + i] = o[k];
    }
}

void ref_acrobot_reset_f32(uint64_t seed, uint64_t lane, uint64_t tick, float state[4]) {
    uint32_t w[4];
    ref_reset_words(seed, lane, tick, w);
    for (int k = 0; k < 4; ++k) state[k] = -0.1f + 0.2f * u01_24(w[k]);
}

/* The Acrobot domain probe of tests/test_env_edge_tables_host.py: every float32 state is stepped three times — upstream semantics in
 * binary64 (unbounded wrap loop), kernel semantics with at most k subtractions in the wrap, and the literal binary32 transcription
 * (the yardstick) — and the facts the domain proof needs come back per lane.  All arrays are structure-of-arrays over n lanes:
 * next64 [4], nextk [4], nextlit [4]; pre64 [3] = the two angles before the wrap and the largest |angle| handed to sin / cos by a stage,
 * prek [3] the same of the twin; wraps64 [2], wrapsk [2] = how often each wrap subtracted; done64 / donek the termination flags. */
void ref_acrobot_domain_probe(const float *state_soa, const int32_t *action, int32_t k, int64_t n,
                              double *next64, float *nextk, float *nextlit, double *pre64, float *prek,
                              int32_t *wraps64, int32_t *wrapsk, uint8_t *done64, uint8_t *donek) {
    for (int64_t i = 0; i < n; ++i) {
        double s64[4], o64[6], r64, p64[3];
        float sk[4], sl[4], ok[6], ol[6], rk, rl, pk[3];
        int w64[2], wk[2];
        for (int c = 0; c < 4; ++c) { sk[c] = sl[c] = state_soa[(int64_t)c * n + i]; s64[c] = (double)sk[c]; }
        done64[i] = (uint8_t)acrobot_step_f64_probe(s64, action[i], o64, &r64, w64, p64);
        donek[i] = (uint8_t)acrobot_step_f32_k(sk, action[i], ok, &rk, k, wk, pk);
        ref_acrobot_step_f32_literal(sl, action[i], ol, &rl);
        for (int c = 0; c < 4; ++c) { next64[(int64_t)c * n + i] = s64[c]; nextk[(int64_t)c * n + i] = sk[c]; nextlit[(int64_t)c * n + i] = sl[c]; }
        for (int c = 0; c < 3; ++c) { pre64[(int64_t)c * n + i] = p64[c]; prek[(int64_t)c * n + i] = pk[c]; }
        for (int c = 0; c < 2; ++c) { wraps64[(int64_t)c * n + i] = w64[c]; wrapsk[(int64_t)c * n + i] = wk[c]; }
    }
}

/* ------------------------------------------------------------------------------------------
 * Batched conveniences over structure-of-arrays [dim][n] for every env (env_id: 0 CartPole, 1 Pendulum,
 * 2 MountainCar, 3 Acrobot), so the parity tests can replay FULL-SIZE (2^20-lane) launches in seconds.
 * They only loop the per-instance functions above; nothing new is restated here except the observation
 * of a freshly reset state (the same sin/cos the step uses).  `action` is int32[n], or float32[n] for Pendulum.
 * ---------------------------------------------------------------------------------------- */
static const int ENV_S[4] = {4, 2, 2, 4};
static const int ENV_O[4] = {4, 3, 2, 6};

int ref_env_state_dim(int env_id) { return (env_id >= 0 && env_id < 4) ? ENV_S[env_id] : -1; }
int ref_env_obs_dim(int env_id) { return (env_id >= 0 && env_id < 4) ? ENV_O[env_id] : -1; }

static void observe_f32(int env_id, const float *s, float *o) {
    switch (env_id) {
        case 0: o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; break;             /* CartPoleEnv.cs:166,185 */
        case 1: ref_sincos_f32_kernel(s[0], &o[1], &o[0]); o[2] = s[1]; break;
        case 2: o[0] = s[0]; o[1] = s[1]; break;
        default: ref_sincos_f32_small(s[0], &o[1], &o[0]); ref_sincos_f32_small(s[1], &o[3], &o[2]); o[4] = s[2]; o[5] = s[3]; break;   /* a FRESH state: the step's own sin/cos */
    }
}

static void reset_f32(int env_id, uint64_t seed, uint64_t lane, uint64_t tick, float *s) {
    switch (env_id) {
        case 0: ref_cartpole_reset_f32(seed, lane, tick, s); break;
        case 1: ref_pendulum_reset_f32(seed, lane, tick, s); break;
        case 2: ref_mountaincar_reset_f32(seed, lane, tick, s); break;
        default: ref_acrobot_reset_f32(seed, lane, tick, s); break;
    }
}

/* one instance, kernel semantics; CartPole with sbd = -1 at entry (what the fused auto-reset guarantees) unless sbd given */
static int step_one_f32(int env_id, float *s, const void *action, int64_t i, int32_t *sbd, float *o, float *reward) {
    int done;
    switch (env_id) {
        case 0: { int b = sbd ? *sbd : -1; done = ref_cartpole_step_f32(s, ((const int32_t *)action)[i], &b, reward); if (sbd) *sbd = b; observe_f32(0, s, o); break; }
        case 1: ref_pendulum_step_f32(s, ((const float *)action)[i], o, reward); done = 0; break;
        case 2: done = ref_mountaincar_step_f32(s, ((const int32_t *)action)[i], reward); observe_f32(2, s, o); break;
        default: done = ref_acrobot_step_f32(s, ((const int32_t *)action)[i], o, reward); break;
    }
    return done;
}

static int step_one_f64(int env_id, double *s, const void *action, int64_t i, int32_t *sbd, double *o, double *reward) {
    int done;
    switch (env_id) {
        case 0: { int b = sbd ? *sbd : -1; float r; done = ref_cartpole_step_f64(s, ((const int32_t *)action)[i], &b, &r); if (sbd) *sbd = b;
                  *reward = r; for (int k = 0; k < 4; ++k) o[k] = s[k]; break; }
        case 1: ref_pendulum_step_f64(s, (double)((const float *)action)[i], o, reward); done = 0; break;
        case 2: done = ref_mountaincar_step_f64(s, ((const int32_t *)action)[i], reward); o[0] = s[0]; o[1] = s[1]; break;
        default: done = ref_acrobot_step_f64(s, ((const int32_t *)action)[i], o, reward); break;
    }
    return done;
}

void ref_env_step_batch_f32(int env_id, float *state_soa, const void *action, int32_t *sbd, float *obs_soa, float *reward,
                            uint8_t *done, int64_t n) {
    const int S = ENV_S[env_id], O = ENV_O[env_id];
    for (int64_t i = 0; i < n; ++i) {
        float s[4], o[6], r;
        for (int k = 0; k < S; ++k) s[k] = state_soa[(int64_t)k * n + i];
        done[i] = (uint8_t)step_one_f32(env_id, s, action, i, sbd ? &sbd[i] : 0, o, &r);
        reward[i] = r;
        for (int k = 0; k < S; ++k) state_soa[(int64_t)k * n + i] = s[k];
        for (int k = 0; k < O; ++k) obs_soa[(int64_t)k * n + i] = o[k];
    }
}

void ref_env_step_batch_f64(int env_id, double *state_soa, const void *action, int32_t *sbd, double *obs_soa, double *reward,
                            uint8_t *done, int64_t n) {
    const int S = ENV_S[env_id], O = ENV_O[env_id];
    for (int64_t i = 0; i < n; ++i) {
        double s[4], o[6], r;
        for (int k = 0; k < S; ++k) s[k] = state_soa[(int64_t)k * n + i];
        done[i] = (uint8_t)step_one_f64(env_id, s, action, i, sbd ? &sbd[i] : 0, o, &r);
        reward[i] = r;
        for (int k = 0; k < S; ++k) state_soa[(int64_t)k * n + i] = s[k];
        for (int k = 0; k < O; ++k) obs_soa[(int64_t)k * n + i] = o[k];
    }
}

void ref_env_reset_batch_f32(int env_id, uint64_t seed, uint64_t lane0, uint64_t tick, float *state_soa, float *obs_soa, int64_t n) {
    const int S = ENV_S[env_id], O = ENV_O[env_id];
    for (int64_t i = 0; i < n; ++i) {
        float s[4], o[6];
        reset_f32(env_id, seed, lane0 + (uint64_t)i, tick, s);
        observe_f32(env_id, s, o);
        for (int k = 0; k < S; ++k) state_soa[(int64_t)k * n + i] = s[k];
        if (obs_soa) for (int k = 0; k < O; ++k) obs_soa[(int64_t)k * n + i] = o[k];
    }
}

/* One vector step as the engine performs it with GYMNET_FLAG_AUTORESET (the caller's `if (done) Reset()`, README.md:36-40,
 * fused): step every lane; reward / done are the step's; a finished lane's state and observation are replaced by the
 * reset draw keyed (seed, lane0 + i, tick).  lane_seed (optional) gives per-lane keys (VecEnv.Seed(int[]), VecEnv.cs:48-52). */
void ref_env_autoreset_step_batch_f32(int env_id, uint64_t seed, const uint64_t *lane_seed, uint64_t lane0, uint64_t tick,
                                      float *state_soa, const void *action, float *obs_soa, float *reward, uint8_t *done, int64_t n) {
    const int S = ENV_S[env_id], O = ENV_O[env_id];
    for (int64_t i = 0; i < n; ++i) {
        float s[4], o[6], r;
        for (int k = 0; k < S; ++k) s[k] = state_soa[(int64_t)k * n + i];
        const int d = step_one_f32(env_id, s, action, i, 0, o, &r);
        if (d) { reset_f32(env_id, lane_seed ? lane_seed[i] : seed, lane0 + (uint64_t)i, tick, s); observe_f32(env_id, s, o); }
        done[i] = (uint8_t)d; reward[i] = r;
        for (int k = 0; k < S; ++k) state_soa[(int64_t)k * n + i] = s[k];
        for (int k = 0; k < O; ++k) obs_soa[(int64_t)k * n + i] = o[k];
    }
}
