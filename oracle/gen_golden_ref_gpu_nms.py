"""Writes tests/golden/ref_gpu_nms.npz: the keep lists of the reference's own CUDA NMS kernel (lib/nms/nms_kernel.cu, hipified and
compiled for gfx950 into oracle/_ref/nms/ by oracle/build_ref.py::build_gpu_nms) on the seeded inputs of tests/test_detect_gpu.py, so
that those tests hold the product against the reference kernel without the reference tree.  Needs a GPU and the oracle/_ref build.

Usage: python oracle/gen_golden_ref_gpu_nms.py [OUT.npz]        (default tests/golden/ref_gpu_nms.npz)"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frcnn_oracle as ora  # noqa: E402
import synth  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "ref_gpu_nms.npz")
# (k, thr, cluster, seed) of test_gpu_rule_bit_exact_vs_the_reference_cuda_kernel; "plain" = random_dets(3000, 11, 12) unmodified
CASES = [(3000, 0.3, 12, 11), (6000, 0.7, 40, 3), (12000, 0.7, 200, 5), (257, 0.5, 3, 2), (64, 0.3, 1, 9)]


def case_key(k, thr, cl, seed):
    return "%d_%g_%d_%d" % (k, thr, cl, seed)


def sorted_dets(d):
    return np.ascontiguousarray(d[ora.order_desc(d[:, 4])])


def digest(ds):
    return hashlib.sha1(np.ascontiguousarray(ds, dtype=np.float32).tobytes()).hexdigest()


def plain_dets():
    return sorted_dets(synth.random_dets(3000, seed=11, cluster=12))


def threshold_case(k, thr, cl, seed):
    return sorted_dets(synth.threshold_dets(k, thr, cl, seed))


def ref_lib(name):
    path = os.path.join(HERE, "_ref", "nms", name)
    if not os.path.exists(path):
        return None
    fn = ctypes.CDLL(path)._Z4_nmsPiS_PKfiifi
    fn.restype = None

    def run(ds, thresh):
        keep = np.zeros(ds.shape[0], dtype=np.int32)
        n = ctypes.c_int(0)
        fn(keep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), np.ascontiguousarray(ds, dtype=np.float32).ctypes.data_as(ctypes.c_void_p),
           ctypes.c_int(ds.shape[0]), ctypes.c_int(ds.shape[1]), ctypes.c_float(thresh), ctypes.c_int(0))
        return keep[:n.value].copy()
    return run


def main(out):
    ref, ref_fma = ref_lib("libref_gpu_nms.so"), ref_lib("libref_gpu_nms_fma.so")
    if ref is None or ref_fma is None:
        raise SystemExit("oracle/_ref/nms not built (python oracle/build_ref.py)")
    arrs = {}
    ds = plain_dets()
    arrs["plain_keep"], arrs["plain_sha1"] = ref(ds, 0.3), np.array(digest(ds))
    for k, thr, cl, seed in CASES:
        key = case_key(k, thr, cl, seed)
        ds = threshold_case(k, thr, cl, seed)
        arrs["keep_" + key], arrs["fma_" + key], arrs["sha1_" + key] = ref(ds, thr), ref_fma(ds, thr), np.array(digest(ds))
        print("%s: kept %d (FMA-contracted build %d)" % (key, arrs["keep_" + key].size, arrs["fma_" + key].size))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrs)
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLD)
