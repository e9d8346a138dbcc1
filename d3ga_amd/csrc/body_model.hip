// body_model.hip -- the SMPL / SMPL-X body model (tetra_sampler.body_model.SMPLlayer, lib/smplman.py:68-74) forward and
// backward for gfx950.  Layouts and the math: include/d3ga.h (d3ga_body_model), d3ga_amd/body_model.py, DESIGN.md sec. 4.
//
// Forward, four launches:
//   pose_fwd    one workgroup per frame: hand PCA -> full pose, Rodrigues, pose feature (R_j - I), rest joints from
//               J0 + Jdirs [beta; psi], forward kinematics level by level in LDS, A_j = [RG_j | tG_j - RG_j J_j].
//   blend_fwd   (element chunk x row chunk) grid over the (NS + 9(J-1), ld) blend directions: per-chunk partial blend
//               offsets of up to 8 frames, so the 61 MB of SMPL-X posedirs are read once per launch, not once per frame.
//   skin_fwd    per vertex: bs = sum of the row-chunk partials (fixed order), T_v = sum_j w_vj A_j over the CSR row,
//               verts = R(Rh) T_v [v_template + bs; 1] + Th.
// Backward, four launches, every reduction into a slab of partials summed in a fixed order (no float atomics: two runs
// give bitwise-equal gradients):
//   skin_bwd    per vertex: dT_v (3x4), dbs_v, and the workgroup's partial of dL/dR(Rh), dL/dTh.
//   blend_bwd   (element chunk x row chunk) grid: partials of dirs . dbs for up to 8 frames.
//   joint_bwd   one workgroup per (joint, frame): dA_j = sum_v w_vj dT_v over the joint's vertex list (CSC).
//   pose_bwd    one workgroup per frame: the partial sums, reverse kinematics, Rodrigues backward, PCA and joint-regression
//               backward.
#include "d3ga_internal.h"
#include "body_model_math.h"
#include "wave_prims.h"

namespace d3ga {

namespace {

constexpr int kMaxJ = D3GA_BODY_MAX_JOINTS;
constexpr int kMaxNS = D3GA_BODY_MAX_SHAPE;
constexpr int kFwdRows = 32;     // rows of the blend directions per blend_fwd workgroup
constexpr int kFwdChunk = 1024;  // elements per blend_fwd workgroup (4 per lane)
constexpr int kBwdRows = 8;      // rows per blend_bwd workgroup
constexpr int kBwdChunk = 2048;  // elements per blend_bwd workgroup (2 x 4 per lane)
constexpr int kMaxFrames = 8;    // frames per blend launch
constexpr int kWaves = kBlock / 64;
constexpr int kSkinBlock = 64;   // per-vertex kernels: 164 workgroups per frame at SMPL-X size, not 41
constexpr int kRtGroups = kBlock / 12;   // pose_bwd: partial sums of the (R(Rh), Th) slab

static_assert(D3GA_BODY_LD_ALIGN % kBwdChunk == 0 && D3GA_BODY_LD_ALIGN % kFwdChunk == 0, "row stride alignment");

// saved per frame (d3ga_body_model_fwd: `saved`): theta 3J | R 9J | RG 9J | tG 3J | Jr 3J | R(Rh) 9 | Rh 3 | Th 3
struct Saved {
    int J;
    __host__ __device__ int theta() const { return 0; }
    __host__ __device__ int R() const { return 3 * J; }
    __host__ __device__ int RG() const { return 12 * J; }
    __host__ __device__ int tG() const { return 21 * J; }
    __host__ __device__ int Jr() const { return 24 * J; }
    __host__ __device__ int Rrh() const { return 27 * J; }
    __host__ __device__ int rh() const { return 27 * J + 9; }
    __host__ __device__ int th() const { return 27 * J + 12; }
};

// Fixed-order sum of N per-lane values over the workgroup; the totals land in out[0..N) (LDS) after the call.
template <int N, int W = kWaves>
__device__ __forceinline__ void block_sum(float (&v)[N], float *red /* W * N */, float *out /* N */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float s = wave_sum(v[i]);
        if (lane == 0) red[w * N + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        float s = 0.f;
        for (int k = 0; k < W; ++k) s += red[k * N + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ int n_coef(const d3ga_body_model &m) { return m.n_shape + m.n_expr; }
__device__ __forceinline__ int n_rows(const d3ga_body_model &m) { return n_coef(m) + 9 * (m.J - 1); }
// A 3J-wide pose is the full layout even when 75 + 2 n_hand_pca is 3J too (45 components): it is always accepted as is.
__device__ __forceinline__ bool compact_layout(const d3ga_body_model &m, int pw) {
    return m.n_hand_pca > 0 && pw == 75 + 2 * m.n_hand_pca && pw != 3 * m.J;
}

// The kinematic tree and the joint shape directions in LDS: the level loops then wait on no global load.
struct TreeLds {
    int lp[kMaxJ + 1], lj[kMaxJ], par[kMaxJ], cp[kMaxJ + 1], cj[kMaxJ];
    float jd[kMaxNS * 3 * kMaxJ];
};
__device__ __forceinline__ void stage_tree(const d3ga_body_model &m, TreeLds &t, bool children) {
    const int J = m.J, tid = threadIdx.x;
    for (int i = tid; i <= m.n_levels; i += kBlock) t.lp[i] = m.level_ptr[i];
    for (int i = tid; i < J; i += kBlock) { t.lj[i] = m.level_joint[i]; t.par[i] = m.parents[i]; }
    if (children) {
        for (int i = tid; i <= J; i += kBlock) t.cp[i] = m.child_ptr[i];
        for (int i = tid; i < J - 1; i += kBlock) t.cj[i] = m.child_joint[i];
    }
    for (int i = tid; i < n_coef(m) * 3 * J; i += kBlock) t.jd[i] = m.Jdirs[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pose_fwd_kernel(d3ga_body_model m, int pw, const float *__restrict__ poses,
                                                          const float *__restrict__ shapes, const float *__restrict__ expr,
                                                          const float *__restrict__ Rh, const float *__restrict__ Th,
                                                          float *__restrict__ coef, float *__restrict__ A,
                                                          float *__restrict__ saved) {
    __shared__ float th[3 * kMaxJ], R[9 * kMaxJ], RG[9 * kMaxJ], tG[3 * kMaxJ], Jr[3 * kMaxJ], c[kMaxNS];
    __shared__ TreeLds tr;
    const int b = blockIdx.x, tid = threadIdx.x, J = m.J, NS = n_coef(m), NR = n_rows(m);
    const Saved S{J};
    stage_tree(m, tr, false);
    float *sv = saved + (size_t)b * D3GA_BODY_SAVED_FLOATS(J);
    float *cf = coef + (size_t)b * NR;
    const float *pose = poses + (size_t)b * pw;
    if (tid < NS) {
        const float x = tid < m.n_shape ? shapes[(size_t)b * m.n_shape + tid]
                                        : (expr ? expr[(size_t)b * m.n_expr + tid - m.n_shape] : 0.f);
        c[tid] = x;
        cf[tid] = x;
    }
    const bool compact = compact_layout(m, pw);
    for (int i = tid; i < 3 * J; i += kBlock) {
        float x;
        if (!compact) {
            x = pose[i];
        } else if (i < 66) {
            x = pose[i];                                           // body
        } else if (i < 75) {
            x = pose[66 + 2 * m.n_hand_pca + (i - 66)];            // jaw, left eye, right eye
        } else {
            const int side = i < 120 ? 0 : 1, k = i - 75 - 45 * side;
            const float *pc = pose + 66 + side * m.n_hand_pca;
            const float *comp = m.hand_comps + (size_t)side * m.n_hand_pca * 45 + k;
            x = m.hand_mean[45 * side + k];
            for (int q = 0; q < m.n_hand_pca; ++q) x += pc[q] * comp[45 * q];
        }
        th[i] = x;
        sv[S.theta() + i] = x;
    }
    __syncthreads();
    if (tid < J) {
        float Rj[9];
        bm::rodrigues(&th[3 * tid], Rj);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            R[9 * tid + i] = Rj[i];
            sv[S.R() + 9 * tid + i] = Rj[i];
        }
        if (tid > 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) cf[NS + 9 * (tid - 1) + i] = Rj[i] - ((i % 4) == 0 ? 1.f : 0.f);
        }
    } else if (tid == kBlock - 1) {
        float r[3] = {Rh ? Rh[3 * b] : 0.f, Rh ? Rh[3 * b + 1] : 0.f, Rh ? Rh[3 * b + 2] : 0.f}, Rr[9];
        bm::rodrigues(r, Rr);
        if (!Rh) {      // no global rotation: exactly the identity (rodrigues(0) is I to f32 rounding only)
#pragma unroll
            for (int i = 0; i < 9; ++i) Rr[i] = (i % 4) == 0 ? 1.f : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) sv[S.Rrh() + i] = Rr[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            sv[S.rh() + i] = r[i];
            sv[S.th() + i] = Th ? Th[3 * b + i] : 0.f;
        }
    }
    __syncthreads();
    for (int i = tid; i < 3 * J; i += kBlock) {
        float x = m.J0[i];
        for (int s = 0; s < NS; ++s) x += c[s] * tr.jd[s * 3 * J + i];
        Jr[i] = x;
        sv[S.Jr() + i] = x;
    }
    __syncthreads();
    for (int L = 0; L < m.n_levels; ++L) {
        const int e = tr.lp[L + 1];
        for (int q = tr.lp[L] + tid; q < e; q += kBlock) {
            const int j = tr.lj[q], p = tr.par[j];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) RG[9 * j + i] = R[9 * j + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) tG[3 * j + i] = Jr[3 * j + i];
            } else {
                const float t[3] = {Jr[3 * j] - Jr[3 * p], Jr[3 * j + 1] - Jr[3 * p + 1], Jr[3 * j + 2] - Jr[3 * p + 2]};
                float Ro[9], to[3];
                bm::compose(&RG[9 * p], &tG[3 * p], &R[9 * j], t, Ro, to);
#pragma unroll
                for (int i = 0; i < 9; ++i) RG[9 * j + i] = Ro[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) tG[3 * j + i] = to[i];
            }
        }
        __syncthreads();
    }
    if (tid < J) {
        const float *g = &RG[9 * tid];
        float rj[3];
        bm::mv3(g, &Jr[3 * tid], rj);
        float *a = A + ((size_t)b * J + tid) * 16;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[4 * r] = g[3 * r]; a[4 * r + 1] = g[3 * r + 1]; a[4 * r + 2] = g[3 * r + 2];
            a[4 * r + 3] = tG[3 * tid + r] - rj[r];
        }
        a[12] = 0.f; a[13] = 0.f; a[14] = 0.f; a[15] = 1.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) sv[S.RG() + 9 * tid + i] = g[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) sv[S.tG() + 3 * tid + i] = tG[3 * tid + i];
    }
}

// bpart[(b * nrc + rc) * ld + e] = sum over the workgroup's rows k of coef[b][k] * dirs[k][e], frames b0 .. b0 + NB
template <int NB>
__global__ __launch_bounds__(kBlock) void blend_fwd_kernel(d3ga_body_model m, int b0, const float *__restrict__ coef,
                                                           float *__restrict__ bpart) {
    __shared__ float cs[kFwdRows * NB];
    const int NR = n_rows(m), rc = blockIdx.y, nrc = gridDim.y, k0 = rc * kFwdRows;
    const int nk = min(kFwdRows, NR - k0);
    for (int i = threadIdx.x; i < nk * NB; i += kBlock) {
        const int b = i / nk, k = i - b * nk;
        cs[k * NB + b] = coef[(size_t)(b0 + b) * NR + k0 + k];
    }
    __syncthreads();
    const size_t e = (size_t)blockIdx.x * kFwdChunk + 4 * threadIdx.x;
    float4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *d = m.dirs + (size_t)k0 * m.ld + e;
#pragma unroll 8
    for (int k = 0; k < nk; ++k) {
        const float4 x = *reinterpret_cast<const float4 *>(d + (size_t)k * m.ld);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float w = cs[k * NB + b];
            acc[b].x += w * x.x; acc[b].y += w * x.y; acc[b].z += w * x.z; acc[b].w += w * x.w;
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
        *reinterpret_cast<float4 *>(bpart + ((size_t)(b0 + b) * nrc + rc) * m.ld + e) = acc[b];
}

__global__ __launch_bounds__(kSkinBlock) void skin_fwd_kernel(d3ga_body_model m, int nrc, const float *__restrict__ bpart,
                                                          const float *__restrict__ A, const float *__restrict__ saved,
                                                          float *__restrict__ verts, float *__restrict__ T,
                                                          float *__restrict__ bs) {
    const int v = blockIdx.x * kSkinBlock + threadIdx.x, b = blockIdx.y, V = m.V, J = m.J;
    if (v >= V) return;
    const Saved S{J};
    const float *sv = saved + (size_t)b * D3GA_BODY_SAVED_FLOATS(J);
    float o[3] = {0.f, 0.f, 0.f};
    const float *bp = bpart + (size_t)b * nrc * m.ld + 3 * (size_t)v;
#pragma unroll 4
    for (int rc = 0; rc < nrc; ++rc) {
        o[0] += bp[(size_t)rc * m.ld]; o[1] += bp[(size_t)rc * m.ld + 1]; o[2] += bp[(size_t)rc * m.ld + 2];
    }
    const size_t vb = (size_t)b * V + v;
    float vp[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        bs[3 * vb + i] = o[i];
        vp[i] = m.v_template[3 * (size_t)v + i] + o[i];
    }
    float t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = 0.f;
    const float *Ab = A + (size_t)b * J * 16;
    for (int q = m.w_ptr[v], qe = m.w_ptr[v + 1]; q < qe; ++q) {
        const float w = m.w_val[q];
        const float *a = Ab + 16 * (size_t)m.w_joint[q];
#pragma unroll
        for (int i = 0; i < 12; ++i) t[i] += w * a[i];
    }
    float4 *To = reinterpret_cast<float4 *>(T + 16 * vb);
    To[0] = make_float4(t[0], t[1], t[2], t[3]);
    To[1] = make_float4(t[4], t[5], t[6], t[7]);
    To[2] = make_float4(t[8], t[9], t[10], t[11]);
    To[3] = make_float4(0.f, 0.f, 0.f, 1.f);
    float u[3], g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = t[4 * r] * vp[0] + t[4 * r + 1] * vp[1] + t[4 * r + 2] * vp[2] + t[4 * r + 3];
    bm::mv3(sv + S.Rrh(), u, g);
#pragma unroll
    for (int i = 0; i < 3; ++i) verts[3 * vb + i] = g[i] + sv[S.th() + i];
}

// ---------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------
// dT (B,V,12), dbs (B,ld) with the tail [3V, ld) zeroed, rtpart (B, gridDim.x, 12): dL/dR(Rh) row-major | dL/dTh
__global__ __launch_bounds__(kSkinBlock) void skin_bwd_kernel(d3ga_body_model m, const float *__restrict__ T,
                                                          const float *__restrict__ bs, const float *__restrict__ saved,
                                                          const float *__restrict__ g_verts, const float *__restrict__ g_T,
                                                          const float *__restrict__ g_bs, float *__restrict__ dT,
                                                          float *__restrict__ dbs, float *__restrict__ rtpart) {
    __shared__ float red[12], tot[12];
    const int v = blockIdx.x * kSkinBlock + threadIdx.x, b = blockIdx.y, V = m.V, J = m.J;
    const Saved S{J};
    const float *sv = saved + (size_t)b * D3GA_BODY_SAVED_FLOATS(J);
    float rt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) rt[i] = 0.f;
    if (v < V) {
        const size_t vb = (size_t)b * V + v;
        const float4 *Tp = reinterpret_cast<const float4 *>(T + 16 * vb);
        const float4 r0 = Tp[0], r1 = Tp[1], r2 = Tp[2];
        const float t[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        float vp[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) vp[i] = m.v_template[3 * (size_t)v + i] + bs[3 * vb + i];
        float gv[3] = {0.f, 0.f, 0.f}, gu[3];
        if (g_verts) {
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] = g_verts[3 * vb + i];
        }
        bm::mtv3(sv + S.Rrh(), gv, gu);
        float u[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) u[r] = t[4 * r] * vp[0] + t[4 * r + 1] * vp[1] + t[4 * r + 2] * vp[2] + t[4 * r + 3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) rt[3 * i + j] = gv[i] * u[j];
            rt[9 + i] = gv[i];
        }
        float d[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            d[4 * r] = gu[r] * vp[0]; d[4 * r + 1] = gu[r] * vp[1]; d[4 * r + 2] = gu[r] * vp[2]; d[4 * r + 3] = gu[r];
        }
        if (g_T) {
            const float4 *gp = reinterpret_cast<const float4 *>(g_T + 16 * vb);
            const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
            d[0] += g0.x; d[1] += g0.y; d[2] += g0.z; d[3] += g0.w;
            d[4] += g1.x; d[5] += g1.y; d[6] += g1.z; d[7] += g1.w;
            d[8] += g2.x; d[9] += g2.y; d[10] += g2.z; d[11] += g2.w;
        }
        float4 *dp = reinterpret_cast<float4 *>(dT + 12 * vb);
        dp[0] = make_float4(d[0], d[1], d[2], d[3]);
        dp[1] = make_float4(d[4], d[5], d[6], d[7]);
        dp[2] = make_float4(d[8], d[9], d[10], d[11]);
        float db[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) db[i] = t[i] * gu[0] + t[4 + i] * gu[1] + t[8 + i] * gu[2];
        if (g_bs) {
#pragma unroll
            for (int i = 0; i < 3; ++i) db[i] += g_bs[3 * vb + i];
        }
        float *o = dbs + (size_t)b * m.ld + 3 * (size_t)v;
        o[0] = db[0]; o[1] = db[1]; o[2] = db[2];
    }
    if (blockIdx.x == 0)
        for (int e = 3 * V + threadIdx.x; e < m.ld; e += kSkinBlock) dbs[(size_t)b * m.ld + e] = 0.f;
    block_sum<12, 1>(rt, red, tot);
    if (threadIdx.x < 12) rtpart[((size_t)b * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = tot[threadIdx.x];
}

// dcpart[((b0 + b) * nec + ec) * NR + k] = sum over the workgroup's elements e of dirs[k][e] * dbs[b0 + b][e]
template <int NB>
__global__ __launch_bounds__(kBlock) void blend_bwd_kernel(d3ga_body_model m, int b0, const float *__restrict__ dbs,
                                                           float *__restrict__ dcpart) {
    __shared__ float red[kWaves * kBwdRows * NB], tot[kBwdRows * NB];
    const int NR = n_rows(m), ec = blockIdx.x, nec = gridDim.x, k0 = blockIdx.y * kBwdRows;
    const int nk = min(kBwdRows, NR - k0);
    const size_t e = (size_t)ec * kBwdChunk + 4 * threadIdx.x;
    float4 g0[NB], g1[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float *p = dbs + (size_t)(b0 + b) * m.ld + e;
        g0[b] = *reinterpret_cast<const float4 *>(p);
        g1[b] = *reinterpret_cast<const float4 *>(p + kBwdChunk / 2);
    }
    float acc[kBwdRows * NB];
#pragma unroll
    for (int r = 0; r < kBwdRows; ++r) {
        float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
        if (r < nk) {
            const float *d = m.dirs + (size_t)(k0 + r) * m.ld + e;
            x0 = *reinterpret_cast<const float4 *>(d);
            x1 = *reinterpret_cast<const float4 *>(d + kBwdChunk / 2);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
            acc[r * NB + b] = ((x0.x * g0[b].x + x0.y * g0[b].y) + (x0.z * g0[b].z + x0.w * g0[b].w)) +
                              ((x1.x * g1[b].x + x1.y * g1[b].y) + (x1.z * g1[b].z + x1.w * g1[b].w));
    }
    block_sum<kBwdRows * NB>(acc, red, tot);
    if (threadIdx.x < nk * NB) {
        const int r = threadIdx.x / NB, b = threadIdx.x - r * NB;
        dcpart[((size_t)(b0 + b) * nec + ec) * NR + k0 + r] = tot[threadIdx.x];
    }
}

// dA[b][j][0..12) = sum over the joint's vertices of w_vj dT_v (+ g_A[b][j][0..12))
__global__ __launch_bounds__(kBlock) void joint_bwd_kernel(d3ga_body_model m, const float *__restrict__ dT,
                                                           const float *__restrict__ g_A, float *__restrict__ dA) {
    __shared__ float red[kWaves * 12], tot[12];
    const int j = blockIdx.x, b = blockIdx.y, V = m.V, J = m.J;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    const float *db = dT + (size_t)b * V * 12;
    for (int q = m.wt_ptr[j] + threadIdx.x, qe = m.wt_ptr[j + 1]; q < qe; q += kBlock) {
        const float w = m.wt_val[q];
        const float4 *p = reinterpret_cast<const float4 *>(db + 12 * (size_t)m.wt_vert[q]);
        const float4 a = p[0], c = p[1], d = p[2];
        acc[0] += w * a.x; acc[1] += w * a.y; acc[2] += w * a.z; acc[3] += w * a.w;
        acc[4] += w * c.x; acc[5] += w * c.y; acc[6] += w * c.z; acc[7] += w * c.w;
        acc[8] += w * d.x; acc[9] += w * d.y; acc[10] += w * d.z; acc[11] += w * d.w;
    }
    block_sum<12>(acc, red, tot);
    if (threadIdx.x < 12) {
        const size_t o = ((size_t)b * J + j);
        dA[o * 12 + threadIdx.x] = tot[threadIdx.x] + (g_A ? g_A[o * 16 + threadIdx.x] : 0.f);
    }
}

__global__ __launch_bounds__(kBlock) void pose_bwd_kernel(d3ga_body_model m, int pw, const float *__restrict__ saved,
                                                          const float *__restrict__ dA, const float *__restrict__ dcpart,
                                                          int nec, const float *__restrict__ rtpart, int nvb,
                                                          float *__restrict__ g_poses, float *__restrict__ g_shapes,
                                                          float *__restrict__ g_expr, float *__restrict__ g_Rh,
                                                          float *__restrict__ g_Th) {
    __shared__ float R[9 * kMaxJ], RG[9 * kMaxJ], Jr[3 * kMaxJ], dR[9 * kMaxJ], dRG[9 * kMaxJ], dtG[3 * kMaxJ],
        dJr[3 * kMaxJ], dth[3 * kMaxJ], dc[kMaxNS], rtp[kBlock], pr[kMaxNS * 12];
    __shared__ TreeLds tr;
    const int b = blockIdx.x, tid = threadIdx.x, J = m.J, NS = n_coef(m), NR = n_rows(m);
    const Saved S{J};
    stage_tree(m, tr, true);
    const float *sv = saved + (size_t)b * D3GA_BODY_SAVED_FLOATS(J);
    for (int i = tid; i < 9 * J; i += kBlock) {
        R[i] = sv[S.R() + i];
        RG[i] = sv[S.RG() + i];
    }
    for (int i = tid; i < 3 * J; i += kBlock) Jr[i] = sv[S.Jr() + i];
    for (int k = tid; k < NR; k += kBlock) {
        float s = 0.f;
#pragma unroll 8
        for (int q = 0; q < nec; ++q) s += dcpart[((size_t)b * nec + q) * NR + k];
        if (k < NS) dc[k] = s;
        else dR[9 + (k - NS)] = s;                // pose feature (R_j - I), j >= 1
    }
    if (tid < 9) dR[tid] = 0.f;
    {   // the (R(Rh), Th) slab: kRtGroups partial sums per value, each over every kRtGroups-th workgroup
        const int i = tid % 12, g = tid / 12;
        float s = 0.f;
        if (g < kRtGroups)
            for (int q = g; q < nvb; q += kRtGroups) s += rtpart[((size_t)b * nvb + q) * 12 + i];
        rtp[tid] = s;
    }
    __syncthreads();
    if (tid < J) {
        // A_j = [RG_j | tG_j - RG_j Jr_j]
        const float *a = dA + ((size_t)b * J + tid) * 12;
        const float dt[3] = {a[3], a[7], a[11]};
        const float *jr = &Jr[3 * tid];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dRG[9 * tid + 3 * r + c] = a[4 * r + c] - dt[r] * jr[c];
            dtG[3 * tid + r] = dt[r];
        }
        float dj[3];
        bm::mtv3(&RG[9 * tid], dt, dj);
#pragma unroll
        for (int i = 0; i < 3; ++i) dJr[3 * tid + i] = -dj[i];
    } else if (tid == kBlock - 1) {
        float rt[12], dr[3];
        for (int i = 0; i < 12; ++i) {
            float s = 0.f;
            for (int g = 0; g < kRtGroups; ++g) s += rtp[12 * g + i];
            rt[i] = s;
        }
        bm::rodrigues_bwd(sv + S.rh(), rt, dr);
        if (g_Rh) {
#pragma unroll
            for (int i = 0; i < 3; ++i) g_Rh[3 * b + i] = dr[i];
        }
        if (g_Th) {
#pragma unroll
            for (int i = 0; i < 3; ++i) g_Th[3 * b + i] = rt[9 + i];
        }
    }
    __syncthreads();
    for (int L = m.n_levels - 1; L >= 0; --L) {
        const int e = tr.lp[L + 1];
        for (int q = tr.lp[L] + tid; q < e; q += kBlock) {
            const int j = tr.lj[q], p = tr.par[j];
            float gRG[9], gt[3], gJ[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) gRG[i] = dRG[9 * j + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) { gt[i] = dtG[3 * j + i]; gJ[i] = dJr[3 * j + i]; }
            const float *rg = &RG[9 * j];
            for (int cq = tr.cp[j], ce = tr.cp[j + 1]; cq < ce; ++cq) {
                const int ch = tr.cj[cq];
                // RG_c = RG_j R_c ; tG_c = RG_j (Jr_c - Jr_j) + tG_j
                const float *rc = &R[9 * ch], *gc = &dRG[9 * ch], *tc = &dtG[3 * ch];
                const float bone[3] = {Jr[3 * ch] - Jr[3 * j], Jr[3 * ch + 1] - Jr[3 * j + 1], Jr[3 * ch + 2] - Jr[3 * j + 2]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        gRG[3 * r + c] += gc[3 * r] * rc[3 * c] + gc[3 * r + 1] * rc[3 * c + 1] + gc[3 * r + 2] * rc[3 * c + 2] +
                                          tc[r] * bone[c];
                float w[3];
                bm::mtv3(rg, tc, w);
#pragma unroll
                for (int i = 0; i < 3; ++i) { gt[i] += tc[i]; gJ[i] -= w[i]; }
            }
            float own[9];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) own[i] = gRG[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) gJ[i] += gt[i];
            } else {
                const float *rp = &RG[9 * p];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        own[3 * r + c] = rp[r] * gRG[c] + rp[3 + r] * gRG[3 + c] + rp[6 + r] * gRG[6 + c];
                float w[3];
                bm::mtv3(rp, gt, w);
#pragma unroll
                for (int i = 0; i < 3; ++i) gJ[i] += w[i];
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) { dRG[9 * j + i] = gRG[i]; dR[9 * j + i] += own[i]; }
#pragma unroll
            for (int i = 0; i < 3; ++i) { dtG[3 * j + i] = gt[i]; dJr[3 * j + i] = gJ[i]; }
        }
        __syncthreads();
    }
    if (tid < J) bm::rodrigues_bwd(sv + S.theta() + 3 * tid, &dR[9 * tid], &dth[3 * tid]);
    __syncthreads();
    // joint regression backward: dc_s += sum_i dJr_i Jdirs[s][i] as 12 strided partial sums per s, added in a fixed order
    for (int t = tid; t < NS * 12; t += kBlock) {
        const int sI = t / 12, q = t - 12 * sI;
        float a = 0.f;
        for (int i = q; i < 3 * J; i += 12) a += dJr[i] * tr.jd[sI * 3 * J + i];
        pr[t] = a;
    }
    __syncthreads();
    if (tid < NS) {
        float s = dc[tid];
        for (int q = 0; q < 12; ++q) s += pr[12 * tid + q];
        if (tid < m.n_shape) {
            if (g_shapes) g_shapes[(size_t)b * m.n_shape + tid] = s;
        } else if (g_expr) {
            g_expr[(size_t)b * m.n_expr + tid - m.n_shape] = s;
        }
    }
    if (!g_poses) return;
    float *gp = g_poses + (size_t)b * pw;
    if (!compact_layout(m, pw)) {
        for (int i = tid; i < 3 * J; i += kBlock) gp[i] = dth[i];
        return;
    }
    const int nh = m.n_hand_pca;
    for (int i = tid; i < pw; i += kBlock) {
        float x;
        if (i < 66) {
            x = dth[i];
        } else if (i < 66 + 2 * nh) {
            const int side = i < 66 + nh ? 0 : 1, q = i - 66 - side * nh;
            const float *comp = m.hand_comps + ((size_t)side * nh + q) * 45;
            const float *d = &dth[75 + 45 * side];
            x = 0.f;
            for (int k = 0; k < 45; ++k) x += d[k] * comp[k];
        } else {
            x = dth[66 + (i - 66 - 2 * nh)];
        }
        gp[i] = x;
    }
}

}  // namespace

static int body_check(const d3ga_body_model *m, int B, int pw) {
    if (!m) return D3GA_E_NULL;
    if (B < 0 || m->V <= 0 || m->J < 2 || m->J > D3GA_BODY_MAX_JOINTS || m->n_shape < 0 || m->n_expr < 0 ||
        m->n_shape + m->n_expr > D3GA_BODY_MAX_SHAPE || m->n_hand_pca < 0 || m->n_hand_pca > 45 || m->n_levels <= 0 ||
        m->n_levels > m->J || m->ld < 3 * m->V || m->ld % D3GA_BODY_LD_ALIGN)
        return D3GA_E_SIZE;
    if (pw != 3 * m->J && !(m->n_hand_pca > 0 && m->J == 55 && pw == 75 + 2 * m->n_hand_pca)) return D3GA_E_CONFIG;
    if (!m->v_template || !m->dirs || !m->w_ptr || !m->w_joint || !m->w_val || !m->wt_ptr || !m->wt_vert || !m->wt_val ||
        !m->J0 || !m->parents || !m->level_ptr || !m->level_joint || !m->child_ptr)
        return D3GA_E_NULL;
    if (m->n_shape + m->n_expr > 0 && !m->Jdirs) return D3GA_E_NULL;
    if (m->J > 1 && !m->child_joint) return D3GA_E_NULL;
    if (pw != 3 * m->J && (!m->hand_comps || !m->hand_mean)) return D3GA_E_NULL;
    return D3GA_OK;
}

struct BodyScratch {
    float *coef, *bpart;                          // forward
    float *dT, *dbs, *rtpart, *dcpart, *dA;       // backward
    int nrc, nec, nvb;
};

static int64_t body_scratch(const d3ga_body_model *m, int B, int pass, void *base, BodyScratch *s) {
    const int64_t NR = m->n_shape + m->n_expr + 9 * (int64_t)(m->J - 1);
    const int nrc = (int)((NR + kFwdRows - 1) / kFwdRows), nec = m->ld / kBwdChunk, nvb = (m->V + kSkinBlock - 1) / kSkinBlock;
    char *p = (char *)base;
    int64_t off = 0;
    auto take = [&](int64_t floats) -> float * {
        float *r = p ? (float *)(p + off) : nullptr;
        off += align256(4 * floats);
        return r;
    };
    BodyScratch t{};
    t.nrc = nrc; t.nec = nec; t.nvb = nvb;
    if (pass == 0) {
        t.coef = take((int64_t)B * NR);
        t.bpart = take((int64_t)B * nrc * m->ld);
    } else {
        t.dT = take((int64_t)B * m->V * 12);
        t.dbs = take((int64_t)B * m->ld);
        t.rtpart = take((int64_t)B * nvb * 12);
        t.dcpart = take((int64_t)B * nec * NR);
        t.dA = take((int64_t)B * m->J * 12);
    }
    if (s) *s = t;
    return off;
}

extern "C" int d3ga_body_model_scratch_bytes(const d3ga_body_model *m, int32_t B, int64_t *fwd_bytes, int64_t *bwd_bytes) {
    if (!m || !fwd_bytes || !bwd_bytes) return D3GA_E_NULL;
    if (B < 0 || m->J <= 0 || m->V <= 0 || m->ld <= 0 || m->ld % D3GA_BODY_LD_ALIGN) return D3GA_E_SIZE;
    *fwd_bytes = body_scratch(m, B, 0, nullptr, nullptr);
    *bwd_bytes = body_scratch(m, B, 1, nullptr, nullptr);
    return D3GA_OK;
}

#define D3GA_BODY_NB_SWITCH(NB, KERNEL, GRID, STREAM, ...)                                                        \
    switch (NB) {                                                                                                 \
        case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 5: hipLaunchKernelGGL(KERNEL<5>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 6: hipLaunchKernelGGL(KERNEL<6>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        case 7: hipLaunchKernelGGL(KERNEL<7>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;              \
        default: hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(kBlock), 0, STREAM, __VA_ARGS__); break;             \
    }

extern "C" int d3ga_body_model_fwd(const d3ga_body_model *m, int32_t B, int32_t pose_width, const float *poses,
                                   const float *shapes, const float *expr, const float *Rh, const float *Th, float *verts,
                                   float *T, float *A, float *bs, float *saved, void *scratch, int64_t scratch_bytes,
                                   d3ga_stream_t stream) {
    D3GA_TRY(body_check(m, B, pose_width));
    if (B == 0) return D3GA_OK;
    if (!poses || (m->n_shape > 0 && !shapes) || !verts || !T || !A || !bs || !saved || !scratch) return D3GA_E_NULL;
    BodyScratch s;
    if (body_scratch(m, B, 0, scratch, &s) > scratch_bytes) return D3GA_E_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_fwd_kernel, dim3(B), dim3(kBlock), 0, st, *m, (int)pose_width, poses, shapes, expr, Rh, Th,
                       s.coef, A, saved);
    const dim3 grid(m->ld / kFwdChunk, s.nrc);
    for (int b0 = 0; b0 < B; b0 += kMaxFrames) {
        const int nb = B - b0 < kMaxFrames ? B - b0 : kMaxFrames;
        D3GA_BODY_NB_SWITCH(nb, blend_fwd_kernel, grid, st, *m, b0, (const float *)s.coef, s.bpart)
    }
    hipLaunchKernelGGL(skin_fwd_kernel, dim3(s.nvb, B), dim3(kSkinBlock), 0, st, *m, s.nrc, (const float *)s.bpart, (const float *)A,
                       (const float *)saved, verts, T, bs);
    return check_launch(st, 0);
}

extern "C" int d3ga_body_model_bwd(const d3ga_body_model *m, int32_t B, int32_t pose_width, const float *saved,
                                   const float *T, const float *bs, const float *g_verts, const float *g_T, const float *g_A,
                                   const float *g_bs, float *g_poses, float *g_shapes, float *g_expr, float *g_Rh,
                                   float *g_Th, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream) {
    D3GA_TRY(body_check(m, B, pose_width));
    if (B == 0) return D3GA_OK;
    if (!saved || !T || !bs || !scratch) return D3GA_E_NULL;
    BodyScratch s;
    if (body_scratch(m, B, 1, scratch, &s) > scratch_bytes) return D3GA_E_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(skin_bwd_kernel, dim3(s.nvb, B), dim3(kSkinBlock), 0, st, *m, T, bs, saved, g_verts, g_T, g_bs, s.dT,
                       s.dbs, s.rtpart);
    const int NR = m->n_shape + m->n_expr + 9 * (m->J - 1);
    const dim3 grid(s.nec, (NR + kBwdRows - 1) / kBwdRows);
    for (int b0 = 0; b0 < B; b0 += kMaxFrames) {
        const int nb = B - b0 < kMaxFrames ? B - b0 : kMaxFrames;
        D3GA_BODY_NB_SWITCH(nb, blend_bwd_kernel, grid, st, *m, b0, (const float *)s.dbs, s.dcpart)
    }
    hipLaunchKernelGGL(joint_bwd_kernel, dim3(m->J, B), dim3(kBlock), 0, st, *m, (const float *)s.dT, g_A, s.dA);
    hipLaunchKernelGGL(pose_bwd_kernel, dim3(B), dim3(kBlock), 0, st, *m, (int)pose_width, saved, (const float *)s.dA,
                       (const float *)s.dcpart, s.nec, (const float *)s.rtpart, s.nvb, g_poses, g_shapes, g_expr, g_Rh, g_Th);
    return check_launch(st, 0);
}

}  // namespace d3ga
