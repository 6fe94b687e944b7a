// orbp_init.cc -- the monocular Initializer (src/Initializer.cc of WChen09/My-SLAM) behind include/orbp.h: the draws, the two
// RANSAC walks, the candidate motions and the acceptance rules on the host, every hypothesis and every CheckRT match through
// orbp_init_body.h, the text the kernels of orbm_init.hip run as well.  Plain C++, no device code.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_init_body.h"
#include "orbp_internal.h"

static int ifail(int code, const char *fmt, ...)
{
    char text[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    orbp_set_error(text);
    return code;
}

static int init_libc_rand(void *) { return rand(); }
static bool g_seeded_once = false;              // DUtils::Random::SeedRandOnce's m_already_seeded (Random.cpp:35-45)

struct InitCheckRT {                            // what one CheckRT call leaves (:798-907)
    int n_good = 0;
    float parallax = 0;
    std::vector<uint8_t> good;                  // vbGood [n1]
    std::vector<float> p3d;                     // vP3D [3 n1]
};

struct orbp_init {
    int n1 = 0, n2 = 0, N = 0, iterations = 0;
    InitCam cam;
    float sigma = 1, sigma2 = 1;
    std::vector<float> keys1, keys2, pn1, pn2;  // mvKeys1 / mvKeys2 (.pt), vPn1 / vPn2 of both Find* calls
    float T1[9], T2[9];
    std::vector<int32_t> m1, m2;                // mvMatches12
    std::vector<float> uv, pn;                  // per match: u1 v1 u2 v2 and the normalised u1 v1 u2 v2
    bool current = false, drawn = false;
    std::vector<int32_t> sets;                  // mvSets [8 iterations]
    int (*rnd)(void *) = init_libc_rand; void *rnd_ctx = nullptr; double rnd_max = RAND_MAX;
    // results of the 2 * iterations hypotheses (H of every set, then F of every set), when attached
    bool att = false;
    std::vector<float> att_sm; std::vector<int32_t> att_cnt; std::vector<uint32_t> att_masks;
    // CheckRT verdicts of n_motions motions, when attached
    int rt_n = 0;
    std::vector<float> rt_Rt, rt_cos, rt_p3d; std::vector<uint8_t> rt_inl, rt_status;

    int words() const { return (N + 31) / 32; }
    int random_int(int lo, int hi)              // DUtils::Random::RandomInt, Random.cpp:47-50
    {
        const int d = hi - lo + 1;
        return int(((double)rnd(rnd_ctx) / (rnd_max + 1.0)) * d) + lo;
    }
    void drop_results() { att = false; att_sm.clear(); att_cnt.clear(); att_masks.clear(); rt_n = 0; }
    bool set_ok(const int32_t *set) const
    {
        for (int j = 0; j < 8; j++)
            if (set[j] < 0 || set[j] >= N) return false;
        return true;
    }
    // one hypothesis: ComputeH21 / ComputeF21 on the set, the products around it, then the Check* pass over every match
    void hypothesis(int model, const int32_t *set, float (&M)[9], float &score, uint8_t *inl, int &count) const
    {
        InitWork wk;
        float v[9], T2x[9];
        for (int j = 0; j < 8; j++) {
            const float *q = &pn[4 * (size_t)set[j]];
            if (model == INIT_MODEL_H) init_fill_h_rows(wk.B, j, q[0], q[1], q[2], q[3]);
            else init_fill_f_row(wk.B, j, q[0], q[1], q[2], q[3]);
        }
        float H12[9];
        if (model == INIT_MODEL_H) {
            init_null_vector(wk, 16, v);
            init_inv33(T2, T2x);
            init_finish_h(v, T1, T2x, M, H12);
        } else {
            init_zero_row(wk.B, 8);
            init_null_vector(wk, 9, v);
            init_transpose33(T2, T2x);
            init_finish_f(v, T1, T2x, wk, M);
        }
        const float inv_s2 = init_inv_sigma2(sigma);
        score = 0;
        count = 0;
        for (int i = 0; i < N; i++) {
            const float *q = &uv[4 * (size_t)i];
            float s1, s2;
            const bool in = model == INIT_MODEL_H ? init_check_h_one(M, H12, q[0], q[1], q[2], q[3], inv_s2, s1, s2)
                                                  : init_check_f_one(M, q[0], q[1], q[2], q[3], inv_s2, s1, s2);
            score += s1;
            score += s2;
            inl[i] = in;
            count += in;
        }
    }
    void check_rt_one_motion(const float *Rt, const uint8_t *inl, uint8_t *status, float *cosp, float *p3d) const
    {
        InitMotion mo;
        init_motion_prepare(cam, Rt, mo);
        const float th2 = (float)(4.0 * (double)sigma2);
        for (int i = 0; i < N; i++) {
            float X[3] = {0, 0, 0}, c = 0;
            int st = INIT_RT_NOT_INLIER;
            const float *q = &uv[4 * (size_t)i];
            if (inl[i]) st = init_check_rt_one(cam, mo, q[0], q[1], q[2], q[3], th2, X, c);
            status[i] = (uint8_t)st; cosp[i] = c;
            memcpy(p3d + 3 * (size_t)i, X, sizeof X);
        }
    }
    // the tail of CheckRT from the per-match verdicts: nGood, vbGood / vP3D at key-1 indices, the parallax (:888-904)
    void collect_rt(const uint8_t *status, const float *cosp, const float *p3d, InitCheckRT &out) const
    {
        out.good.assign(n1, 0);
        out.p3d.assign(3 * (size_t)n1, 0.f);
        out.n_good = 0;
        std::vector<float> vcos;
        for (int i = 0; i < N; i++) {
            if (status[i] > INIT_RT_GOOD_LOW_PARALLAX) {
                if (status[i] == INIT_RT_NOT_FINITE) out.good[m1[i]] = 0;    // :843
                continue;
            }
            vcos.push_back(cosp[i]);
            memcpy(&out.p3d[3 * (size_t)m1[i]], p3d + 3 * (size_t)i, 3 * sizeof(float));
            out.n_good++;
            if (status[i] == INIT_RT_GOOD) out.good[m1[i]] = 1;
        }
        if (out.n_good > 0) {
            std::sort(vcos.begin(), vcos.end());
            const size_t idx = std::min(50, int(vcos.size() - 1));
            out.parallax = (float)((double)(acosf(vcos[idx]) * 180) / 3.1415926535897932384626433832795);
        } else
            out.parallax = 0;
    }
    void check_rt(int k, const float *Rt, const uint8_t *inl, InitCheckRT &out) const
    {
        // attached verdicts count only for the very motion and flags they were computed for
        if (k < rt_n && !memcmp(&rt_Rt[12 * (size_t)k], Rt, 12 * sizeof(float)) && (N == 0 || !memcmp(rt_inl.data(), inl, N))) {
            collect_rt(&rt_status[(size_t)k * N], &rt_cos[(size_t)k * N], &rt_p3d[3 * (size_t)k * N], out);
            return;
        }
        std::vector<uint8_t> st(std::max(N, 1));
        std::vector<float> c(std::max(N, 1)), p(3 * (size_t)std::max(N, 1));
        check_rt_one_motion(Rt, inl, st.data(), c.data(), p.data());
        collect_rt(st.data(), c.data(), p.data(), out);
    }
    // FindHomography / FindFundamental's walk (:148-171 / :199-222): returns the winning iteration or -1
    int find(int model, float (&M)[9], float &score, uint8_t *inl) const
    {
        score = 0.0f;
        for (int i = 0; i < N; i++) inl[i] = 0;
        for (int i = 0; i < 9; i++) M[i] = 0.f;
        int win = -1;
        std::vector<uint8_t> cur(std::max(N, 1));
        const size_t W = (size_t)words();
        for (int it = 0; it < iterations; it++) {
            float Mi[9], sc;
            if (att) {
                const size_t h = (size_t)(model == INIT_MODEL_H ? it : iterations + it);
                sc = att_sm[10 * h];
                if (!(sc > score)) continue;
                memcpy(Mi, &att_sm[10 * h + 1], sizeof Mi);
                for (int i = 0; i < N; i++) cur[i] = (att_masks[W * h + (i >> 5)] >> (i & 31)) & 1u;
            } else {
                int cnt;
                hypothesis(model, &sets[8 * (size_t)it], Mi, sc, cur.data(), cnt);
            }
            if (sc > score) {
                memcpy(M, Mi, sizeof Mi);
                if (N) memcpy(inl, cur.data(), N);
                score = sc;
                win = it;
            }
        }
        return win;
    }
};

extern "C" int orbp_init_create(orbp_init **out, const float *keys1, int n1, float fx, float fy, float cx, float cy, float sigma, int iterations)
{
    if (!out) return ifail(ORBX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n1 < 0 || iterations < 0 || (n1 > 0 && !keys1)) return ifail(ORBX_E_INVALID, "bad reference frame");
    if (iterations > (1 << 20)) return ifail(ORBX_E_CAPACITY, "more than 2^20 iterations");
    orbp_init *s = new orbp_init();
    s->n1 = n1;
    if (n1) s->keys1.assign(keys1, keys1 + 2 * (size_t)n1);
    s->cam = {fx, fy, cx, cy};
    s->sigma = sigma; s->sigma2 = sigma * sigma;
    s->iterations = iterations;
    *out = s;
    return 0;
}

extern "C" void orbp_init_destroy(orbp_init *s) { delete s; }

extern "C" void orbp_init_set_rand(orbp_init *s, int (*fn)(void *), void *ctx, int rand_max)
{
    if (!s) return;
    if (fn) { s->rnd = fn; s->rnd_ctx = ctx; s->rnd_max = rand_max; }
    else { s->rnd = init_libc_rand; s->rnd_ctx = nullptr; s->rnd_max = RAND_MAX; }
}

extern "C" int orbp_init_set_current(orbp_init *s, const float *keys2, int n2, const int32_t *matches12)
{
    if (!s || n2 < 0 || (n2 > 0 && !keys2) || (s->n1 > 0 && !matches12)) return ifail(ORBX_E_INVALID, "bad current frame");
    for (int i = 0; i < s->n1; i++)
        if (matches12[i] >= n2) return ifail(ORBX_E_INVALID, "matches12[%d] = %d outside the %d current keys", i, matches12[i], n2);
    s->n2 = n2;
    s->keys2.assign(keys2, keys2 + 2 * (size_t)n2);
    s->m1.clear(); s->m2.clear();
    for (int i = 0; i < s->n1; i++)             // :54-63
        if (matches12[i] >= 0) { s->m1.push_back(i); s->m2.push_back(matches12[i]); }
    const int N = s->N = (int)s->m1.size();
    s->pn1.assign(2 * (size_t)s->n1, 0.f); s->pn2.assign(2 * (size_t)n2, 0.f);
    init_normalize(s->keys1.data(), s->n1, s->pn1.data(), s->T1);      // :132-133 / :183-184: the same in both threads
    init_normalize(s->keys2.data(), n2, s->pn2.data(), s->T2);
    s->uv.resize(4 * (size_t)N); s->pn.resize(4 * (size_t)N);
    for (int i = 0; i < N; i++) {
        const size_t a = 2 * (size_t)s->m1[i], b = 2 * (size_t)s->m2[i];
        float *u = &s->uv[4 * (size_t)i], *p = &s->pn[4 * (size_t)i];
        u[0] = s->keys1[a]; u[1] = s->keys1[a + 1]; u[2] = s->keys2[b]; u[3] = s->keys2[b + 1];
        p[0] = s->pn1[a]; p[1] = s->pn1[a + 1]; p[2] = s->pn2[b]; p[3] = s->pn2[b + 1];
    }
    s->current = true; s->drawn = false;
    s->sets.clear();
    s->drop_results();
    return N;
}

extern "C" int orbp_init_draw(orbp_init *s, int32_t *sets)
{
    if (!s) return ifail(ORBX_E_INVALID, "solver is NULL");
    if (!s->current) return ifail(ORBX_E_INVALID, "no current frame");
    if (s->N < 8) return ifail(ORBX_E_INVALID, "%d matches: a minimal set needs 8", s->N);
    if (s->rnd == init_libc_rand && !g_seeded_once) { srand(0); g_seeded_once = true; }     // SeedRandOnce(0) :80
    s->sets.assign(8 * (size_t)s->iterations, 0);
    s->drop_results();
    std::vector<int32_t> avail;
    for (int it = 0; it < s->iterations; it++) {                // :82-97
        avail.resize(s->N);
        for (int i = 0; i < s->N; i++) avail[i] = i;
        for (int j = 0; j < 8; j++) {
            const int r = s->random_int(0, (int)avail.size() - 1);
            s->sets[8 * (size_t)it + j] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    s->drawn = true;
    if (sets && s->iterations) memcpy(sets, s->sets.data(), s->sets.size() * sizeof(int32_t));
    return s->iterations;
}

extern "C" int orbp_init_get_sizes(const orbp_init *s, int *n1, int *n2, int *n_matches, int *iterations, int *drawn)
{
    if (!s) return ifail(ORBX_E_INVALID, "solver is NULL");
    if (n1) *n1 = s->n1;
    if (n2) *n2 = s->n2;
    if (n_matches) *n_matches = s->N;
    if (iterations) *iterations = s->iterations;
    if (drawn) *drawn = s->drawn ? 1 : 0;
    return 0;
}

extern "C" int orbp_init_get_problem(const orbp_init *s, float *uv, float *pn, float *params, int32_t *sets, int32_t *m1, int32_t *m2)
{
    if (!s || !s->current) return ifail(ORBX_E_INVALID, "no current frame");
    const size_t N = (size_t)s->N;
    if (uv && N) memcpy(uv, s->uv.data(), 16 * N);
    if (pn && N) memcpy(pn, s->pn.data(), 16 * N);
    if (params) {
        memcpy(params, s->T1, sizeof s->T1); memcpy(params + 9, s->T2, sizeof s->T2);
        params[18] = s->sigma; params[19] = s->cam.fx; params[20] = s->cam.fy; params[21] = s->cam.cx; params[22] = s->cam.cy;
        params[23] = (float)(4.0 * (double)s->sigma2);
    }
    if (sets && s->drawn && s->iterations) memcpy(sets, s->sets.data(), s->sets.size() * sizeof(int32_t));
    if (m1 && N) memcpy(m1, s->m1.data(), 4 * N);
    if (m2 && N) memcpy(m2, s->m2.data(), 4 * N);
    return s->N;
}

extern "C" int orbp_init_normalized(const orbp_init *s, float *pn1, float *T1, float *pn2, float *T2)
{
    if (!s || !s->current) return ifail(ORBX_E_INVALID, "no current frame");
    if (pn1 && s->n1) memcpy(pn1, s->pn1.data(), 8 * (size_t)s->n1);
    if (pn2 && s->n2) memcpy(pn2, s->pn2.data(), 8 * (size_t)s->n2);
    if (T1) memcpy(T1, s->T1, sizeof s->T1);
    if (T2) memcpy(T2, s->T2, sizeof s->T2);
    return 0;
}

extern "C" int orbp_init_hypothesis(const orbp_init *s, int model, const int32_t *set, float *M, float *score, uint8_t *inliers, int *n_inliers)
{
    if (!s || !set || !M || !score || !n_inliers || (s->N > 0 && !inliers)) return ifail(ORBX_E_INVALID, "NULL argument");
    if (!s->current) return ifail(ORBX_E_INVALID, "no current frame");
    if (model != INIT_MODEL_H && model != INIT_MODEL_F) return ifail(ORBX_E_INVALID, "model %d is neither H (0) nor F (1)", model);
    if (!s->set_ok(set)) return ifail(ORBX_E_INVALID, "set index outside [0, %d)", s->N);
    float Mi[9];
    s->hypothesis(model, set, Mi, *score, inliers, *n_inliers);
    memcpy(M, Mi, sizeof Mi);
    return 0;
}

extern "C" int orbp_init_attach_results(orbp_init *s, int n_hyp, const float *score_M, const int32_t *counts, const uint32_t *masks)
{
    if (!s || n_hyp < 0) return ifail(ORBX_E_INVALID, "bad arguments");
    if (!s->drawn) return ifail(ORBX_E_INVALID, "nothing drawn");
    if (n_hyp != 2 * s->iterations) return ifail(ORBX_E_INVALID, "%d results for %d sets of two models", n_hyp, s->iterations);
    const size_t W = (size_t)s->words(), H = (size_t)n_hyp;
    if (H > 0 && (!score_M || !counts || (W > 0 && !masks))) return ifail(ORBX_E_INVALID, "NULL argument");
    s->att_sm.assign(score_M, score_M + 10 * H);
    s->att_cnt.assign(counts, counts + H);
    s->att_masks.assign(masks, masks + W * H);
    s->att = true;
    return 0;
}

extern "C" int orbp_init_find(orbp_init *s, int model, float *M, float *score, uint8_t *inliers, int *best_iteration)
{
    if (!s || !M || !score || (s->N > 0 && !inliers)) return ifail(ORBX_E_INVALID, "NULL argument");
    if (model != INIT_MODEL_H && model != INIT_MODEL_F) return ifail(ORBX_E_INVALID, "model %d is neither H (0) nor F (1)", model);
    if (!s->drawn) return ifail(ORBX_E_INVALID, "nothing drawn");
    float Mi[9];
    const int win = s->find(model, Mi, *score, inliers);
    memcpy(M, Mi, sizeof Mi);
    if (best_iteration) *best_iteration = win;
    return win >= 0 ? 1 : 0;
}

extern "C" int orbp_init_motions(const orbp_init *s, int model, const float *M, float *Rt, int *n_motions)
{
    if (!s || !M || !Rt || !n_motions) return ifail(ORBX_E_INVALID, "NULL argument");
    if (model != INIT_MODEL_H && model != INIT_MODEL_F) return ifail(ORBX_E_INVALID, "model %d is neither H (0) nor F (1)", model);
    InitWork wk;
    float Mi[9];
    memcpy(Mi, M, sizeof Mi);
    *n_motions = 0;
    if (model == INIT_MODEL_F) { init_motions_f(Mi, s->cam, wk, Rt); *n_motions = 4; return 1; }
    float tmp[96];
    if (!init_motions_h(Mi, s->cam, wk, tmp)) return 0;
    memcpy(Rt, tmp, sizeof tmp);
    *n_motions = 8;
    return 1;
}

extern "C" int orbp_init_check_rt_matches(const orbp_init *s, int n_motions, const float *Rt, const uint8_t *inliers, uint8_t *status,
                                          float *cos_parallax, float *p3d)
{
    if (!s || !s->current || n_motions < 0) return ifail(ORBX_E_INVALID, "bad arguments");
    if (n_motions > 0 && s->N > 0 && (!Rt || !inliers || !status || !cos_parallax || !p3d)) return ifail(ORBX_E_INVALID, "NULL argument");
    for (int k = 0; k < n_motions; k++)
        s->check_rt_one_motion(Rt + 12 * (size_t)k, inliers, status + (size_t)k * s->N, cos_parallax + (size_t)k * s->N, p3d + 3 * (size_t)k * s->N);
    return 0;
}

extern "C" int orbp_init_check_rt(const orbp_init *s, const float *R, const float *t, const uint8_t *inliers, float *p3d, uint8_t *good,
                                  float *parallax, int *n_good)
{
    if (!s || !R || !t || !parallax || !n_good || (s->N > 0 && !inliers) || (s->n1 > 0 && (!p3d || !good))) return ifail(ORBX_E_INVALID, "NULL argument");
    if (!s->current) return ifail(ORBX_E_INVALID, "no current frame");
    float Rt[12];
    memcpy(Rt, R, 36); memcpy(Rt + 9, t, 12);
    InitCheckRT out;
    s->check_rt(1 << 30, Rt, inliers, out);     // never from attached verdicts: this is the host's own answer
    if (s->n1) { memcpy(p3d, out.p3d.data(), 12 * (size_t)s->n1); memcpy(good, out.good.data(), s->n1); }
    *parallax = out.parallax; *n_good = out.n_good;
    return 0;
}

extern "C" int orbp_init_attach_check_rt(orbp_init *s, int n_motions, const float *Rt, const uint8_t *inliers, const uint8_t *status,
                                         const float *cos_parallax, const float *p3d)
{
    if (!s || !s->current || n_motions < 0 || n_motions > 8) return ifail(ORBX_E_INVALID, "bad arguments");
    const size_t N = (size_t)s->N, K = (size_t)n_motions;
    if (K > 0 && (!Rt || (N > 0 && (!inliers || !status || !cos_parallax || !p3d)))) return ifail(ORBX_E_INVALID, "NULL argument");
    for (size_t i = 0; i < K * N; i++)
        if (status[i] > INIT_RT_REPROJ2) return ifail(ORBX_E_INVALID, "status %d at %zu", status[i], i);
    s->rt_Rt.assign(Rt, Rt + 12 * K);
    s->rt_inl.assign(inliers, inliers + (K ? N : 0));
    s->rt_status.assign(status, status + K * N);
    s->rt_cos.assign(cos_parallax, cos_parallax + K * N);
    s->rt_p3d.assign(p3d, p3d + 3 * K * N);
    s->rt_n = n_motions;
    return 0;
}

// Initialize up to the CheckRT calls (:99-118, :473-497 / :575-686): which model is reconstructed, its matrix, its inlier flags and
// its candidate motions.  Returns the number of motions (0: nothing to reconstruct)
static int init_plan(orbp_init *s, int &model, float (&M)[9], std::vector<uint8_t> &inl, float (&Rt)[96])
{
    const int N = s->N;
    std::vector<uint8_t> inlH(std::max(N, 1)), inlF(std::max(N, 1));
    float H[9], F[9], SH, SF;
    s->find(INIT_MODEL_H, H, SH, inlH.data());
    s->find(INIT_MODEL_F, F, SF, inlF.data());
    const float RH = SH / (SH + SF);            // :112
    if (RH != RH) return 0;                     // SH == SF == 0: the reference decomposes an empty matrix; refused here (orbp.h)
    InitWork wk;
    if ((double)RH > 0.40) {
        model = INIT_MODEL_H; memcpy(M, H, sizeof H); inl = inlH;
        return init_motions_h(M, s->cam, wk, Rt) ? 8 : 0;
    }
    model = INIT_MODEL_F; memcpy(M, F, sizeof F); inl = inlF;
    init_motions_f(M, s->cam, wk, Rt);
    return 4;
}

extern "C" int orbp_init_plan_check_rt(orbp_init *s, int *model, float *M, uint8_t *inliers, float *Rt, int *n_motions)
{
    if (!s || !model || !M || !Rt || !n_motions || (s->N > 0 && !inliers)) return ifail(ORBX_E_INVALID, "NULL argument");
    if (!s->drawn) return ifail(ORBX_E_INVALID, "nothing drawn");
    float Mi[9] = {0}, R[96];
    std::vector<uint8_t> inl;
    int mdl = -1;
    const int n = init_plan(s, mdl, Mi, inl, R);
    *model = mdl; *n_motions = n;
    memcpy(M, Mi, sizeof Mi);
    if (n) { memcpy(Rt, R, 48 * (size_t)n); if (s->N) memcpy(inliers, inl.data(), s->N); }
    return n;
}

extern "C" int orbp_init_initialize(orbp_init *s, float *R21, float *t21, float *p3d, uint8_t *triangulated)
{
    if (!s || !R21 || !t21 || (s->n1 > 0 && (!p3d || !triangulated))) return ifail(ORBX_E_INVALID, "NULL argument");
    if (!s->current) return ifail(ORBX_E_INVALID, "no current frame");
    if (!s->drawn) {
        const int rc = orbp_init_draw(s, nullptr);
        if (rc < 0) return rc;
    }
    float M[9] = {0}, Rt[96];
    std::vector<uint8_t> inl;
    int model = -1;
    const int nm = init_plan(s, model, M, inl, Rt);
    if (nm == 0) return 0;
    int N = 0;                                  // :473-476 / :575-578
    for (int i = 0; i < s->N; i++) N += inl[i];
    const float minParallax = 1.0f;
    const int minTriangulated = 50;
    InitCheckRT rt[8];
    for (int k = 0; k < nm; k++) s->check_rt(k, Rt + 12 * k, inl.data(), rt[k]);
    int best = -1;
    if (model == INIT_MODEL_F) {                // :499-569
        const int g1 = rt[0].n_good, g2 = rt[1].n_good, g3 = rt[2].n_good, g4 = rt[3].n_good;
        const int maxGood = std::max(g1, std::max(g2, std::max(g3, g4)));
        const int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);
        int nsimilar = 0;
        if (g1 > 0.7 * maxGood) nsimilar++;
        if (g2 > 0.7 * maxGood) nsimilar++;
        if (g3 > 0.7 * maxGood) nsimilar++;
        if (g4 > 0.7 * maxGood) nsimilar++;
        if (maxGood < nMinGood || nsimilar > 1) return 0;
        const int k = maxGood == g1 ? 0 : maxGood == g2 ? 1 : maxGood == g3 ? 2 : 3;
        if (rt[k].parallax > minParallax) best = k;
    } else {                                    // :689-729
        int bestGood = 0, secondBestGood = 0, bestIdx = -1;
        float bestParallax = -1;
        for (int i = 0; i < 8; i++) {
            const int nGood = rt[i].n_good;
            if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; bestIdx = i; bestParallax = rt[i].parallax; }
            else if (nGood > secondBestGood) secondBestGood = nGood;
        }
        if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) best = bestIdx;
    }
    if (best < 0) return 0;
    memcpy(R21, Rt + 12 * best, 36); memcpy(t21, Rt + 12 * best + 9, 12);
    if (s->n1) { memcpy(p3d, rt[best].p3d.data(), 12 * (size_t)s->n1); memcpy(triangulated, rt[best].good.data(), s->n1); }
    return 1;
}
