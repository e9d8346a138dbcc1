// skeleton.hip -- the momentum-style skeleton of the Goliath body model (lbsmodel/body_model.py: ParameterTransform,
// solve_skeleton_state, states_to_matrix, the root transform) forward and backward for gfx950.  Layouts: include/d3ga.h
// (d3ga_skeleton), d3ga_amd/skeleton_model.py; per-joint math: skeleton_math.h.
//
//   skeleton_fwd   one workgroup per (frame, scale set): skeleton parameters = CSR(transform) . [poses; scales] + offsets (columns
//                  ascending: a fixed sum order), local transforms, the parent -> child chain level by level in LDS, then per
//                  joint the state, the 4x4 matrix against the bind state and the root joint's (R, t).  Scale set 0 reads
//                  `scales`, every further set reads zeros: the posed solve and the zero-scale root solve share the launch.
//   skeleton_bwd   one workgroup per frame, the sets one after the other: dL/d(state) of every joint from dL/d(mats, root,
//                  states), the reverse chain (deepest level first, each joint gathering its children in CSR order), local
//                  transform and Euler backward, then the transposed parameter transform as a CSC (rows ascending).  No float
//                  atomics anywhere: two calls give bitwise-equal gradients.
//   skeleton_mats_fwd / _bwd   one thread per (frame, joint): states -> matrices for callers that hold states of their own.
#include "d3ga_internal.h"
#include "skeleton_math.h"

namespace d3ga {

namespace {

constexpr int kSkMaxJ = D3GA_SKEL_MAX_JOINTS;
constexpr int kSaved = D3GA_SKEL_SAVED_FLOATS;      // per joint: local state 8 | Euler angles 3 | 0

struct SkelTree {
    int lp[kSkMaxJ + 1], lj[kSkMaxJ], par[kSkMaxJ];
};

__device__ __forceinline__ void stage_tree(const d3ga_skeleton &m, SkelTree &t) {
    for (int i = threadIdx.x; i <= m.n_levels; i += kBlock) t.lp[i] = m.level_ptr[i];
    for (int i = threadIdx.x; i < m.J; i += kBlock) { t.lj[i] = m.level_joint[i]; t.par[i] = m.parents[i]; }
}

__global__ __launch_bounds__(kBlock) void skeleton_fwd_kernel(d3ga_skeleton m, int B, int pw, const float *__restrict__ poses,
                                                              const float *__restrict__ scales, int scale_rows,
                                                              const float *__restrict__ direct, const float *__restrict__ bind,
                                                              float trans_scale, int root_joint, float *__restrict__ states,
                                                              float *__restrict__ saved, float *__restrict__ mats,
                                                              float *__restrict__ root) {
    __shared__ float st[8 * kSkMaxJ], loc[8 * kSkMaxJ];
    __shared__ SkelTree tr;
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, J = m.J, ns = m.n_params - pw;
    const size_t fb = (size_t)s * B + b;
    stage_tree(m, tr);
    // skeleton parameters, staged in st (free until the chain starts)
    const float *pose = poses ? poses + (size_t)b * pw : nullptr;
    const float *sc = (s == 0 && scales) ? scales + (size_t)(scale_rows == 1 ? 0 : b) * ns : nullptr;
    for (int r = tid; r < 7 * J; r += kBlock) {
        float x;
        if (direct) {
            x = direct[(size_t)b * 7 * J + r];
        } else {
            float acc = 0.f;
            const int e = m.csr_ptr[r + 1];
            for (int k = m.csr_ptr[r]; k < e; ++k) {
                const int c = m.csr_col[k];
                const float v = c < pw ? pose[c] : (sc ? sc[c - pw] : 0.f);
                acc += m.csr_val[k] * v;
            }
            x = acc + m.transform_offsets[r];
        }
        st[r] = x;
    }
    __syncthreads();
    for (int j = tid; j < J; j += kBlock) {
        float p[7], l[8];
#pragma unroll
        for (int i = 0; i < 7; ++i) p[i] = st[7 * j + i];
        sk::local_state(p, m.joint_offset + 3 * j, m.joint_rotation + 4 * j, l);
        float *sv = saved + (fb * J + j) * kSaved;
#pragma unroll
        for (int i = 0; i < 8; ++i) { loc[8 * j + i] = l[i]; sv[i] = l[i]; }
        sv[8] = p[3]; sv[9] = p[4]; sv[10] = p[5]; sv[11] = 0.f;
    }
    __syncthreads();
    for (int L = 0; L < m.n_levels; ++L) {
        const int e = tr.lp[L + 1];
        for (int q = tr.lp[L] + tid; q < e; q += kBlock) {
            const int j = tr.lj[q], p = tr.par[j];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) st[8 * j + i] = loc[8 * j + i];
            } else {
                float P[8], l[8], o[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) { P[i] = st[8 * p + i]; l[i] = loc[8 * j + i]; }
                sk::chain_step(P, l, o);
#pragma unroll
                for (int i = 0; i < 8; ++i) st[8 * j + i] = o[i];
            }
        }
        __syncthreads();
    }
    for (int j = tid; j < J; j += kBlock) {
        float S[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) S[i] = st[8 * j + i];
        float *so = states + (fb * J + j) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) so[i] = S[i];
        if (bind) {
            float bj[8], binv[8], M[12];
#pragma unroll
            for (int i = 0; i < 8; ++i) bj[i] = bind[8 * j + i];
            sk::bind_inverse(bj, binv);
            sk::joint_matrix(binv, S, M);
            if (mats) {
                float *a = mats + (fb * J + j) * 16;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    a[4 * r] = M[4 * r]; a[4 * r + 1] = M[4 * r + 1]; a[4 * r + 2] = M[4 * r + 2];
                    a[4 * r + 3] = M[4 * r + 3] * trans_scale;
                }
                a[12] = 0.f; a[13] = 0.f; a[14] = 0.f; a[15] = 1.f;
            }
            if (root && j == root_joint) {
                float *ro = root + fb * 12;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    ro[3 * r] = M[4 * r]; ro[3 * r + 1] = M[4 * r + 1]; ro[3 * r + 2] = M[4 * r + 2];
                    ro[9 + r] = M[4 * r + 3];
                }
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void skeleton_bwd_kernel(d3ga_skeleton m, int B, int n_sets, int pw, int direct_mode,
                                                              const float *__restrict__ bind, float trans_scale, int root_joint,
                                                              const float *__restrict__ states, const float *__restrict__ saved,
                                                              const float *__restrict__ g_states, const float *__restrict__ g_mats,
                                                              const float *__restrict__ g_root, float *__restrict__ g_poses,
                                                              float *__restrict__ g_scales, float *__restrict__ g_direct) {
    __shared__ float st[8 * kSkMaxJ], loc[8 * kSkMaxJ], ds[8 * kSkMaxJ];
    __shared__ SkelTree tr;
    __shared__ int cp[kSkMaxJ + 1], cj[kSkMaxJ];
    const int b = blockIdx.x, tid = threadIdx.x, J = m.J, ns = m.n_params - pw;
    stage_tree(m, tr);
    for (int i = tid; i <= J; i += kBlock) cp[i] = m.child_ptr[i];
    for (int i = tid; i < m.n_children; i += kBlock) cj[i] = m.child_joint[i];
    for (int s = n_sets - 1; s >= 0; --s) {
        const size_t fb = (size_t)s * B + b;
        __syncthreads();                    // the previous set is done with the LDS arrays (and the tables are staged)
        for (int j = tid; j < J; j += kBlock) {
            float S[8], g[8];
            const float *so = states + (fb * J + j) * 8, *sv = saved + (fb * J + j) * kSaved;
#pragma unroll
            for (int i = 0; i < 8; ++i) { S[i] = so[i]; st[8 * j + i] = S[i]; loc[8 * j + i] = sv[i]; }
#pragma unroll
            for (int i = 0; i < 8; ++i) g[i] = g_states ? g_states[(fb * J + j) * 8 + i] : 0.f;
            const bool is_root = g_root && j == root_joint;
            if (bind && (g_mats || is_root)) {
                float bj[8], binv[8], G[12], d[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) bj[i] = bind[8 * j + i];
                sk::bind_inverse(bj, binv);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        G[4 * r + c] = (g_mats ? g_mats[(fb * J + j) * 16 + 4 * r + c] : 0.f) + (is_root ? g_root[fb * 12 + 3 * r + c] : 0.f);
                    G[4 * r + 3] = (g_mats ? g_mats[(fb * J + j) * 16 + 4 * r + 3] * trans_scale : 0.f) + (is_root ? g_root[fb * 12 + 9 + r] : 0.f);
                }
                sk::joint_matrix_bwd(binv, S, G, d);
#pragma unroll
                for (int i = 0; i < 8; ++i) g[i] += d[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ds[8 * j + i] = g[i];
        }
        __syncthreads();
        // reverse chain: the leaves of the deepest level have nothing to gather
        for (int L = m.n_levels - 2; L >= 0; --L) {
            const int e = tr.lp[L + 1];
            for (int q = tr.lp[L] + tid; q < e; q += kBlock) {
                const int j = tr.lj[q], ce = cp[j + 1];
                if (cp[j] == ce) continue;
                float P[8], acc[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) { P[i] = st[8 * j + i]; acc[i] = ds[8 * j + i]; }
                for (int k = cp[j]; k < ce; ++k) {
                    const int c = cj[k];
                    float l[8], g[8], dP[8], dl[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { l[i] = loc[8 * c + i]; g[i] = ds[8 * c + i]; }
                    sk::chain_step_bwd(P, l, g, dP, dl);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { acc[i] += dP[i]; loc[8 * c + i] = dl[i]; }    // loc[c] now holds dL/d(local c)
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) ds[8 * j + i] = acc[i];
            }
            __syncthreads();
        }
        // local transform backward; dL/d(skeleton parameters) of joint j lands in ds[8j .. 8j+7)
        for (int j = tid; j < J; j += kBlock) {
            float dl[8], l[8] = {}, p[7], dp[7];
            const bool is_tree_root = tr.par[j] < 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) dl[i] = is_tree_root ? ds[8 * j + i] : loc[8 * j + i];
            const float *sv = saved + (fb * J + j) * kSaved;
            p[0] = p[1] = p[2] = p[6] = 0.f;
            p[3] = sv[8]; p[4] = sv[9]; p[5] = sv[10];
            l[7] = sv[7];
            sk::local_state_bwd(p, m.joint_rotation + 4 * j, l, dl, dp);
#pragma unroll
            for (int i = 0; i < 7; ++i) ds[8 * j + i] = dp[i];
        }
        __syncthreads();
        if (direct_mode) {
            if (g_direct)
                for (int r = tid; r < 7 * J; r += kBlock) g_direct[(size_t)b * 7 * J + r] = ds[8 * (r / 7) + r % 7];
        } else {
            for (int p = tid; p < m.n_params; p += kBlock) {
                const bool is_pose = p < pw;
                if (!is_pose && s > 0) continue;                    // the scales of the further sets are constants (zero)
                float *dst = is_pose ? (g_poses ? g_poses + (size_t)b * pw + p : nullptr)
                                     : (g_scales ? g_scales + (size_t)b * ns + (p - pw) : nullptr);
                if (!dst) continue;
                float acc = 0.f;
                const int e = m.csc_ptr[p + 1];
                for (int k = m.csc_ptr[p]; k < e; ++k) {
                    const int r = m.csc_row[k];
                    acc += m.csc_val[k] * ds[8 * (r / 7) + r % 7];
                }
                const bool first = is_pose ? (s == n_sets - 1) : true;
                *dst = first ? acc : *dst + acc;
            }
        }
    }
}

// states -> matrices against a bind state, one thread per (frame, joint): the free-standing form of the forward's last step
__global__ __launch_bounds__(kBlock) void skeleton_mats_fwd_kernel(int n, int J, const float *__restrict__ bind,
                                                                   const float *__restrict__ states, float *__restrict__ mats) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = i % J;
    float bj[8], binv[8], S[8], M[12];
#pragma unroll
    for (int k = 0; k < 8; ++k) { bj[k] = bind[8 * j + k]; S[k] = states[(size_t)i * 8 + k]; }
    sk::bind_inverse(bj, binv);
    sk::joint_matrix(binv, S, M);
    float *a = mats + (size_t)i * 16;
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = M[k];
    a[12] = 0.f; a[13] = 0.f; a[14] = 0.f; a[15] = 1.f;
}

__global__ __launch_bounds__(kBlock) void skeleton_mats_bwd_kernel(int n, int J, const float *__restrict__ bind,
                                                                   const float *__restrict__ states,
                                                                   const float *__restrict__ g_mats, float *__restrict__ g_states) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = i % J;
    float bj[8], binv[8], S[8], G[12], d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { bj[k] = bind[8 * j + k]; S[k] = states[(size_t)i * 8 + k]; }
#pragma unroll
    for (int k = 0; k < 12; ++k) G[k] = g_mats[(size_t)i * 16 + k];
    sk::bind_inverse(bj, binv);
    sk::joint_matrix_bwd(binv, S, G, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) g_states[(size_t)i * 8 + k] = d[k];
}

}  // namespace

extern "C" int d3ga_skeleton_mats_fwd(int32_t B, int32_t J, const float *bind, const float *states, float *mats,
                                      d3ga_stream_t stream) {
    if (B < 0 || J <= 0 || (int64_t)B * J > INT32_MAX) return D3GA_E_SIZE;
    if (B == 0) return D3GA_OK;
    if (!bind || !states || !mats) return D3GA_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    const int n = B * J;
    hipLaunchKernelGGL(skeleton_mats_fwd_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (int)J, bind, states, mats);
    return check_launch(st, 0);
}

extern "C" int d3ga_skeleton_mats_bwd(int32_t B, int32_t J, const float *bind, const float *states, const float *g_mats,
                                      float *g_states, d3ga_stream_t stream) {
    if (B < 0 || J <= 0 || (int64_t)B * J > INT32_MAX) return D3GA_E_SIZE;
    if (B == 0) return D3GA_OK;
    if (!bind || !states || !g_mats || !g_states) return D3GA_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    const int n = B * J;
    hipLaunchKernelGGL(skeleton_mats_bwd_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (int)J, bind, states, g_mats,
                       g_states);
    return check_launch(st, 0);
}

extern "C" int d3ga_skeleton_check(const d3ga_skeleton *m, int32_t B, int32_t n_sets, int32_t pose_width) {
    if (!m) return D3GA_E_NULL;
    if (B < 0 || n_sets < 1 || m->J < 2 || m->J > D3GA_SKEL_MAX_JOINTS || m->n_params < 0 || m->n_levels <= 0 || m->n_levels > m->J ||
        m->n_children < 0 || m->n_children >= m->J || pose_width < 0 || pose_width > m->n_params)
        return D3GA_E_SIZE;
    if (!m->parents || !m->level_ptr || !m->level_joint || !m->child_ptr || !m->child_joint || !m->joint_offset ||
        !m->joint_rotation || !m->transform_offsets || !m->csr_ptr || !m->csr_col || !m->csr_val || !m->csc_ptr || !m->csc_row ||
        !m->csc_val)
        return D3GA_E_NULL;
    return D3GA_OK;
}

extern "C" int d3ga_skeleton_fwd(const d3ga_skeleton *m, int32_t B, int32_t n_sets, int32_t pose_width, const float *poses,
                                 const float *scales, int32_t scale_rows, const float *direct, const float *bind,
                                 float trans_scale, int32_t root_joint, float *states, float *saved, float *mats, float *root,
                                 d3ga_stream_t stream) {
    D3GA_TRY(d3ga_skeleton_check(m, B, n_sets, pose_width));
    if (B == 0) return D3GA_OK;
    if (!states || !saved) return D3GA_E_NULL;
    if (direct ? n_sets != 1 : (pose_width > 0 && !poses)) return direct ? D3GA_E_CONFIG : D3GA_E_NULL;
    if (scales && scale_rows != 1 && scale_rows != B) return D3GA_E_SIZE;
    if ((mats || root) && !bind) return D3GA_E_NULL;
    if (root && (root_joint < 0 || root_joint >= m->J)) return D3GA_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(skeleton_fwd_kernel, dim3(B, n_sets), dim3(kBlock), 0, st, *m, (int)B, (int)pose_width, poses, scales,
                       (int)scale_rows, direct, bind, trans_scale, (int)root_joint, states, saved, mats, root);
    return check_launch(st, 0);
}

extern "C" int d3ga_skeleton_bwd(const d3ga_skeleton *m, int32_t B, int32_t n_sets, int32_t pose_width, int32_t direct_mode,
                                 const float *bind, float trans_scale, int32_t root_joint, const float *states,
                                 const float *saved, const float *g_states, const float *g_mats, const float *g_root,
                                 float *g_poses, float *g_scales, float *g_direct, d3ga_stream_t stream) {
    D3GA_TRY(d3ga_skeleton_check(m, B, n_sets, pose_width));
    if (B == 0) return D3GA_OK;
    if (!states || !saved) return D3GA_E_NULL;
    if (direct_mode && n_sets != 1) return D3GA_E_CONFIG;
    if ((g_mats || g_root) && !bind) return D3GA_E_NULL;
    if (g_root && (root_joint < 0 || root_joint >= m->J)) return D3GA_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(skeleton_bwd_kernel, dim3(B), dim3(kBlock), 0, st, *m, (int)B, (int)n_sets, (int)pose_width,
                       (int)direct_mode, bind, trans_scale, (int)root_joint, states, saved, g_states, g_mats, g_root, g_poses,
                       g_scales, g_direct);
    return check_launch(st, 0);
}

}  // namespace d3ga
