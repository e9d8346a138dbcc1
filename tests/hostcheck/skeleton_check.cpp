// Host build of d3ga_amd/csrc/skeleton_math.h for tests/test_skeleton_host.py: every function behind a C entry point, arrays in
// and out as the header takes them.
#include "../../d3ga_amd/csrc/skeleton_math.h"

using namespace d3ga::sk;

extern "C" {
void sk_qmul(const float *a, const float *b, float *o) { qmul(a, b, o); }
void sk_qmul_bwd(const float *a, const float *b, const float *g, float *da, float *db) { qmul_bwd(a, b, g, da, db); }
void sk_qrot(const float *q, const float *v, float *o) { qrot(q, v, o); }
void sk_qrot_bwd(const float *q, const float *v, const float *g, float *dq, float *dv) { qrot_bwd(q, v, g, dq, dv); }
void sk_euler_quat(const float *r, float *q) { euler_quat(r, q); }
void sk_euler_quat_bwd(const float *r, const float *g, float *dr) { euler_quat_bwd(r, g, dr); }
void sk_local_state(const float *p, const float *off, const float *pre, float *l) { local_state(p, off, pre, l); }
void sk_local_state_bwd(const float *p, const float *pre, const float *l, const float *g, float *dp) { local_state_bwd(p, pre, l, g, dp); }
void sk_chain_step(const float *P, const float *l, float *o) { chain_step(P, l, o); }
void sk_chain_step_bwd(const float *P, const float *l, const float *g, float *dP, float *dl) { chain_step_bwd(P, l, g, dP, dl); }
void sk_bind_inverse(const float *b, float *o) { bind_inverse(b, o); }
void sk_joint_matrix(const float *bind, const float *s, float *M) {
    float binv[8];
    bind_inverse(bind, binv);
    joint_matrix(binv, s, M);
}
void sk_joint_matrix_bwd(const float *bind, const float *s, const float *G, float *ds) {
    float binv[8];
    bind_inverse(bind, binv);
    joint_matrix_bwd(binv, s, G, ds);
}
}
