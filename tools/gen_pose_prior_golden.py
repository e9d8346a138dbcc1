"""Record tests/golden/pose_prior_cases.npz from the reference's own build_pca and transform_pca on the CPU (scikit-learn).

    python tools/gen_pose_prior_golden.py --reference /path/to/reference

The reference is read at generation time only and none of its text is kept: `build_pca` is loaded from its
utils/pca_utils.py (loguru, which is not installed, is stubbed in sys.modules), and `transform_pca` is taken out of test.py by
parsing it with `ast` and compiling that one function (test.py itself calls .cuda() at module level and cannot be imported).
The fixture holds numeric arrays only.

Per case (N, D, k) of tests/pose_prior_ref.CASES, key prefix "c<i>_":
    x (N,D) f32, poses (5,D) f32              the data (pose_prior_ref.make_case)
    variance (k) f64                           scikit-learn's explained_variance_ on float64 input
    z (5,k) f64, proj (5,D) f64                its transform and inverse_transform(transform) of the poses
    out (3,5,D) f64                            the reference's transform_pca at sigma = 1.5, 2.0, 3.0 on float64 input
    out32 (3,5,D) f64                          the same with float32 input all the way: the reference's own arithmetic
    clamped (3,5,k) bool                       which coefficients the clip changed
    route (2,) f64                             measured: |Gram + eigh route - SVD oracle| and |scikit-learn f64 - SVD oracle|,
                                               each as a share of max|out|; asserted here: their sum <= 0.25 * 2^-23
"""
import argparse
import ast
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def load_reference(path):
    if "loguru" not in sys.modules:
        stub = types.ModuleType("loguru")
        stub.logger = types.SimpleNamespace(info=lambda *a, **k: None)
        sys.modules["loguru"] = stub
    spec = importlib.util.spec_from_file_location("_ref_pca_utils", os.path.join(path, "utils", "pca_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(path, "test.py")) as f:
        tree = ast.parse(f.read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "transform_pca")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "<transform_pca>", "exec"), ns)
    return mod.build_pca, ns["transform_pca"]


def gram_route(x, poses, k, sigma):
    """what PosePCA does in float64 numpy: covariance, eigh, the k largest pairs, clip, back-project"""
    import pose_prior_ref as R
    from d3ga_amd.pose_prior import _decompose
    mean, cov = R.covariance(x)
    comp, var = _decompose(mean, cov, k)
    return R.clamp((mean, comp, var), poses, sigma)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pose_prior_cases.npz"))
    args = ap.parse_args()
    import pose_prior_ref as R
    build_pca, transform_pca = load_reference(args.reference)
    data = {}
    for i, (n, d, k) in enumerate(R.CASES):
        x, poses = R.make_case(n, d, k, seed=100 + i)
        x64, p64 = x.astype(np.float64), poses.astype(np.float64)
        pca = build_pca("", list(x64), n_components=k, save=False)
        assert pca._fit_svd_solver != "randomized", (n, d, k, pca._fit_svd_solver)
        pca32 = build_pca("", list(x), n_components=k, save=False)
        basis = R.fit(x64, k)
        out = np.stack([np.stack([transform_pca(pca, p, sigma_pca=s) for p in p64]) for s in R.SIGMAS])
        out32 = np.stack([np.stack([transform_pca(pca32, p, sigma_pca=s) for p in poses]) for s in R.SIGMAS]).astype(np.float64)
        oracle = np.stack([R.clamp(basis, p64, s)[0] for s in R.SIGMAS])
        clamped = np.stack([R.clamp(basis, p64, s)[1] for s in R.SIGMAS])
        gram = np.stack([gram_route(x64, p64, k, s) for s in R.SIGMAS])
        scale = np.abs(oracle).max()
        route = np.array([np.abs(gram - oracle).max() / scale, np.abs(out - oracle).max() / scale])
        assert route.sum() <= 0.25 * R.BAR, (n, d, k, route)
        if n >= 3 and k >= 2:                               # a condition on the data, not a tolerance
            both = clamped.any(axis=2) & ~clamped.all(axis=2)
            assert both.any(axis=1).all(), (n, d, k, "no pose with clamped and unclamped coefficients at some sigma")
        z = pca.transform(p64)
        data.update({f"c{i}_x": x, f"c{i}_poses": poses, f"c{i}_variance": pca.explained_variance_, f"c{i}_z": z,
                     f"c{i}_proj": pca.inverse_transform(z), f"c{i}_out": out, f"c{i}_out32": out32, f"c{i}_clamped": clamped,
                     f"c{i}_route": route})
        print(f"({n},{d},{k}) solver={pca._fit_svd_solver} route gram {route[0]:.2e} sklearn {route[1]:.2e} "
              f"f32 gap {np.abs(out32 - out).max() / scale:.2e} clamped {clamped.mean():.2f}")
    data["shapes"] = np.array(R.CASES, dtype=np.int32)
    data["sigmas"] = np.array(R.SIGMAS, dtype=np.float64)
    np.savez_compressed(args.out, **data)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
