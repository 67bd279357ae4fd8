// Host check of the posterior comparison's per-voxel arithmetic (ir_sgmcmc_amd/csrc/compare_device.h, the header the kernel
// compiles).  Stand-alone: its own main, nothing of it is loaded into Python.
//
//   compare_check                 the known answers, then seeded random pairs of covariances in double -- general, rank-deficient,
//                                 near-isotropic and 1e+-20-scaled -- against closed forms and invariants.  Prints, per quantity,
//                                 the worst error in units of the bound forms of tests/_posterior_comparison.py with c = 1
//                                 (bures^2: 2^-26 (tr S_A + tr S_B); jeffreys: 2^-53 * the sum of the absolute values of its
//                                 terms), and `violations N`: the count of exact properties that did not hold.
//   compare_check eval IN OUT     evaluates compare_maps on the float32 states of the file IN and writes the planes to OUT
//                                 (layouts below): how the tests hold the host build to the numpy restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ir_sgmcmc_amd/csrc/compare_device.h"

using irs::CompareCore;
using irs::compare_core;

static int violations = 0;
static double worst_bures = 0.0, worst_jeffreys = 0.0, worst_jeffreys_inputs = 0.0, worst_log = 0.0, worst_known = 0.0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        ++violations;
        std::printf("VIOLATION: %s\n", what);
    }
}

struct Sym {
    double a[6];  // a00, a11, a22, a01, a02, a12
};

static void to_full(const Sym& s, double (&m)[3][3]) {
    m[0][0] = s.a[0], m[1][1] = s.a[1], m[2][2] = s.a[2];
    m[0][1] = m[1][0] = s.a[3], m[0][2] = m[2][0] = s.a[4], m[1][2] = m[2][1] = s.a[5];
}

// Q diag(l) Q^T
static Sym compose(const double (&Q)[3][3], const double (&l)[3]) {
    double m[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = Q[i][0] * l[0] * Q[j][0] + Q[i][1] * l[1] * Q[j][1] + Q[i][2] * l[2] * Q[j][2];
    return Sym{{m[0][0], m[1][1], m[2][2], m[0][1], m[0][2], m[1][2]}};
}

// Q S Q^T
static Sym rotate(const double (&Q)[3][3], const Sym& s) {
    double m[3][3], t[3][3], r[3][3];
    to_full(s, m);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i][j] = Q[i][0] * m[0][j] + Q[i][1] * m[1][j] + Q[i][2] * m[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i][j] = t[i][0] * Q[j][0] + t[i][1] * Q[j][1] + t[i][2] * Q[j][2];
    return Sym{{r[0][0], r[1][1], r[2][2], 0.5 * (r[0][1] + r[1][0]), 0.5 * (r[0][2] + r[2][0]), 0.5 * (r[1][2] + r[2][1])}};
}

template <class Rng>
static void random_rotation(Rng& rng, double (&Q)[3][3]) {
    std::uniform_real_distribution<double> ang(-M_PI, M_PI);
    const double a = ang(rng), b = ang(rng), c = ang(rng);
    const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b), cc = std::cos(c), sc = std::sin(c);
    Q[0][0] = ca * cb, Q[0][1] = ca * sb * sc - sa * cc, Q[0][2] = ca * sb * cc + sa * sc;
    Q[1][0] = sa * cb, Q[1][1] = sa * sb * sc + ca * cc, Q[1][2] = sa * sb * cc - ca * sc;
    Q[2][0] = -sb, Q[2][1] = cb * sc, Q[2][2] = cb * cc;
}

static CompareCore core(const Sym& A, const Sym& B, const double (&d)[3], double floor2) { return compare_core(A.a, B.a, d, floor2); }

static double bures_unit(const CompareCore& c) { return std::ldexp(c.tr_a + c.tr_b, -26); }
static double jeffreys_unit(const CompareCore& c) { return std::ldexp(c.terms, -53); }
// where the two sides of a check see inputs rounded differently (a rotated or a composed matrix: eps |S| per entry, which moves
// a floored eigenvalue f by up to eps tr S, a relative eps tr S / f of every term it enters)
static double jeffreys_inputs_unit(const CompareCore& c, const double (&la)[3], const double (&lb)[3], double floor2) {
    double fa = INFINITY, fb = INFINITY;
    for (int i = 0; i < 3; ++i) fa = std::fmin(fa, std::fmax(la[i], floor2)), fb = std::fmin(fb, std::fmax(lb[i], floor2));
    return jeffreys_unit(c) * (1.0 + c.tr_a / fa + c.tr_b / fb);
}

static void track(double& worst, double err, double unit) {
    if (unit > 0.0 && err / unit > worst) worst = err / unit;
    if (!(unit > 0.0) && err > 0.0) worst = INFINITY;
}

static void known(const char* name, const Sym& A, const double (&ma)[3], const Sym& B, const double (&mb)[3], double shift,
                  double half_log, double bures2, double jeffreys, int floored) {
    const double d[3] = {ma[0] - mb[0], ma[1] - mb[1], ma[2] - mb[2]};
    const CompareCore c = core(A, B, d, 1e-6);
    std::printf("known %-22s shift %.17g log_std_ratio %.17g bures2 %.17g jeffreys %.17g floored %d\n", name, std::sqrt(c.shift2),
                c.half_log, c.bures2, c.jeffreys, (int)c.floored);
    track(worst_known, std::fabs(std::sqrt(c.shift2) - shift), std::ldexp(std::fmax(shift, 1.0), -50));
    track(worst_known, std::fabs(c.half_log - half_log), std::ldexp(1.0, -50));
    track(worst_bures, std::fabs(c.bures2 - bures2), bures_unit(c));
    track(worst_jeffreys, std::fabs(c.jeffreys - jeffreys), jeffreys_unit(c));
    expect((int)c.floored == floored, "known answer: the floored flag");
}

static int self_check() {
    const double r = std::sqrt(0.5), zero[3] = {0, 0, 0};
    const Sym I{{1, 1, 1, 0, 0, 0}}, D{{4, 1, 0.25, 0, 0, 0}};
    {
        const double ma[3] = {1, 2, 2};
        known("diagonal", D, ma, I, zero, 3.0, 0.5 * std::log(5.25 / 3.0), 1.25, 16.875, 0);
        const double Q[3][3] = {{r, -r, 0}, {r, r, 0}, {0, 0, 1}};
        known("rotated", rotate(Q, D), zero, I, zero, 0.0, 0.5 * std::log(5.25 / 3.0), 1.25, 2.25, 0);
        // 1/2 [4 / f^2 + 9 / f^2 + 2 (f^2 / f^2) ... ]: tr(B~^-1 A~) = 4e6 + 1e-6 / 9 + 1, tr(A~^-1 B~) = 1e-6 / 4 + 9e6 + 1
        const Sym A1{{4, 0, 0, 0, 0, 0}}, B1{{0, 9, 0, 0, 0, 0}};
        known("rank one, orthogonal", A1, zero, B1, zero, 0.0, 0.5 * std::log(4.0 / 9.0), 13.0,
              0.5 * (4e6 + 1e-6 / 9 + 1 + 1e-6 / 4 + 9e6 + 1 - 6), 1);
        const Sym S = rotate(Q, Sym{{2.5, 0.7, 0.01, 0, 0, 0}});
        const CompareCore c = core(S, S, zero, 1e-6);  // identical states
        expect(c.shift2 == 0.0, "identical states: shift exactly 0");
        expect(c.half_log == 0.0, "identical states: log_std_ratio exactly 0");
        track(worst_bures, c.bures2, bures_unit(c));
        track(worst_jeffreys, std::fabs(c.jeffreys), jeffreys_unit(c));
    }

    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::normal_distribution<double> nrm(0.0, 1.0);
    const int kinds = 5, per_kind = 800;
    for (int kind = 0; kind < kinds; ++kind) {
        for (int it = 0; it < per_kind; ++it) {
            double QA[3][3], QB[3][3], la[3], lb[3], d[3];
            random_rotation(rng, QA);
            random_rotation(rng, QB);
            for (int i = 0; i < 3; ++i) {
                la[i] = std::exp(3.0 * nrm(rng)), lb[i] = std::exp(3.0 * nrm(rng));
                d[i] = nrm(rng);
            }
            double floor2 = 1e-6, s = 1.0;
            if (kind == 1) {  // rank-deficient: one or two exact zeros on either side
                la[it % 3] = 0.0;
                if (it % 2) lb[(it / 3) % 3] = 0.0;
                if (it % 5 == 0) la[(it + 1) % 3] = 0.0;
            } else if (kind == 2) {  // near-isotropic: the eigenvalues within 1e-9 of one another
                for (int i = 0; i < 3; ++i) la[i] = 2.0 * (1.0 + 1e-9 * uni(rng)), lb[i] = 0.5 * (1.0 + 1e-12 * uni(rng));
            } else if (kind == 3) {  // everything scaled by 1e+20 (covariances by 1e+40)
                s = 1e20;
            } else if (kind == 4) {  // everything scaled by 1e-20: below any floor
                s = 1e-20;
            }
            for (int i = 0; i < 3; ++i) la[i] *= s * s, lb[i] *= s * s, d[i] *= s;
            const Sym A = compose(QA, la), B = compose(QB, lb);
            const double md[3] = {-d[0], -d[1], -d[2]};
            const CompareCore ab = core(A, B, d, floor2), ba = core(B, A, md, floor2);
            // finite, non-negative
            expect(std::isfinite(ab.bures2) && std::isfinite(ab.jeffreys) && std::isfinite(ab.half_log), "finite outputs");
            expect(ab.bures2 >= 0.0, "bures^2 >= 0");
            track(worst_jeffreys, std::fmax(-ab.jeffreys, 0.0), jeffreys_unit(ab));  // >= 0 within the bound
            // symmetry / antisymmetry under A <-> B
            expect(ab.half_log == -ba.half_log, "log_std_ratio exactly antisymmetric");
            expect(ab.shift2 == ba.shift2, "shift exactly symmetric");
            expect(ab.floored == ba.floored, "floored symmetric");
            track(worst_bures, std::fabs(ab.bures2 - ba.bures2), bures_unit(ab));
            track(worst_jeffreys, std::fabs(ab.jeffreys - ba.jeffreys), jeffreys_unit(ab));
            // identical inputs
            const double z[3] = {0, 0, 0};
            const CompareCore aa = core(A, A, z, floor2);
            expect(aa.shift2 == 0.0 && aa.half_log == 0.0, "identical inputs: shift and log_std_ratio exactly 0");
            track(worst_bures, aa.bures2, bures_unit(aa));
            track(worst_jeffreys, std::fabs(aa.jeffreys), jeffreys_unit(aa));
            // a common rotation
            double Q[3][3];
            random_rotation(rng, Q);
            double qd[3];
            for (int i = 0; i < 3; ++i) qd[i] = Q[i][0] * d[0] + Q[i][1] * d[1] + Q[i][2] * d[2];
            const CompareCore rot = core(rotate(Q, A), rotate(Q, B), qd, floor2);
            // the rotated matrices are rounded entry by entry: eps |S| of perturbation each, which the bound forms cover
            track(worst_bures, std::fabs(rot.bures2 - ab.bures2), bures_unit(ab));
            track(worst_jeffreys_inputs, std::fabs(rot.jeffreys - ab.jeffreys), jeffreys_inputs_unit(ab, la, lb, floor2));
            track(worst_log, std::fabs(rot.half_log - ab.half_log), std::ldexp(1.0, -50));
            // closed forms.  Commuting pair (B built on A's axes): bures^2 = sum (sqrt la - sqrt lb)^2, jeffreys by eigenvalue
            const Sym Bc = compose(QA, lb);
            const CompareCore cm = core(A, Bc, z, floor2);
            double b2 = 0.0, je = 0.0;
            for (int i = 0; i < 3; ++i) {
                b2 += (std::sqrt(la[i]) - std::sqrt(lb[i])) * (std::sqrt(la[i]) - std::sqrt(lb[i]));
                const double fa = std::fmax(la[i], floor2), fb = std::fmax(lb[i], floor2);
                je += 0.5 * (fa / fb + fb / fa - 2.0);
            }
            track(worst_bures, std::fabs(cm.bures2 - b2), bures_unit(cm));
            track(worst_jeffreys_inputs, std::fabs(cm.jeffreys - je), jeffreys_inputs_unit(cm, la, lb, floor2));
        }
    }
    std::printf("worst known %.6g\nworst log_std_ratio %.6g\nworst bures %.6g\nworst jeffreys %.6g\nworst jeffreys, rounded inputs %.6g\n",
                worst_known, worst_log, worst_bures, worst_jeffreys, worst_jeffreys_inputs);
    std::printf("violations %d\n", violations);
    return violations ? 1 : 0;
}

// IN:  int64 V, n_a, n_b; double scale[3], std_floor; float32 mean_a[3 V], comoment_a[6 V], mean_b[3 V], comoment_b[6 V]
// OUT: float32 shift[V], log_std_ratio[V], bures[V], jeffreys[V]; double tr_a[V], tr_b[V]; uint8 finite[V], floored[V]
static int eval(const char* in_path, const char* out_path) {
    std::FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    int64_t head[3];
    double par[4];
    if (std::fread(head, 8, 3, f) != 3 || std::fread(par, 8, 4, f) != 4 || head[0] < 1) return 2;
    const size_t V = (size_t)head[0];
    std::vector<float> st(18 * V);
    if (std::fread(st.data(), 4, 18 * V, f) != 18 * V) return 2;
    std::fclose(f);
    const float *mean_a = st.data(), *com_a = mean_a + 3 * V, *mean_b = com_a + 6 * V, *com_b = mean_b + 3 * V;
    std::vector<float> planes(4 * V);
    std::vector<double> tr(2 * V);
    std::vector<uint8_t> flags(2 * V);
    const double sc[3] = {par[0], par[1], par[2]}, floor2 = par[3] * par[3];
    const double inv_a = 1.0 / (double)(head[1] - 1), inv_b = 1.0 / (double)(head[2] - 1);
    for (size_t v = 0; v < V; ++v) {
        float mu_a[3], M_a[6], mu_b[3], M_b[6];
        for (int c = 0; c < 3; ++c) mu_a[c] = mean_a[c * V + v], mu_b[c] = mean_b[c * V + v];
        for (int c = 0; c < 6; ++c) M_a[c] = com_a[c * V + v], M_b[c] = com_b[c * V + v];
        const irs::CompareMaps o = irs::compare_maps(mu_a, M_a, inv_a, mu_b, M_b, inv_b, sc, floor2);
        planes[v] = o.shift, planes[V + v] = o.log_std_ratio, planes[2 * V + v] = o.bures, planes[3 * V + v] = o.jeffreys;
        tr[v] = o.tr_a, tr[V + v] = o.tr_b;
        flags[v] = o.finite, flags[V + v] = o.floored;
    }
    std::FILE* g = std::fopen(out_path, "wb");
    if (!g) return 2;
    const bool ok = std::fwrite(planes.data(), 4, 4 * V, g) == 4 * V && std::fwrite(tr.data(), 8, 2 * V, g) == 2 * V &&
                    std::fwrite(flags.data(), 1, 2 * V, g) == 2 * V;
    return std::fclose(g) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "eval") == 0) return eval(argv[2], argv[3]);
    if (argc == 1) return self_check();
    std::fprintf(stderr, "usage: %s [eval IN OUT]\n", argv[0]);
    return 2;
}
