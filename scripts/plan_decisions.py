#!/usr/bin/env python3
"""Snapshot of every decision a plan takes, over a fixed matrix of plans (tests/test_plan_decisions_*.py compare against it).

  python scripts/plan_decisions.py --device -1 --out tests/golden/plan_decisions_host.json
  python scripts/plan_decisions.py --device 0  --out tests/golden/plan_decisions_gpu.json

Host matrix (device = -1): per plan the return code, the error text of a refused plan, otherwise every integer field of nufft_info
(sigma and beta as hex floats) and the nufft_plan_options text.  Device matrix: in addition the workspace and its breakdown, and for
five fixed-seed point sets (uniform; folded N(0, 1) three times; 24 points per bin) the engines and the sort that served each —
the stream is synchronised after every set_points, so the host-mapped feedback of the adaptive sort has arrived before the next one.

The file holds the plans in the matrix's order, column by column and run-length encoded (encode / decode below).
The golden files are recorded with the library of the commit BEFORE a change to the decision code and must not be re-recorded to make
such a change pass.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TYPES = (("f32r", 0, 0), ("f32c", 0, 1), ("f64r", 1, 0), ("f64c", 1, 1))      # name, dtype, is_complex
SWITCHES = ("NUFFT_SMARCH_HALO=0", "NUFFT_SMARCH_HALO=2", "NUFFT_SMARCH_SPLIT=0", "NUFFT_INTERP_SPLIT=0", "NUFFT_INTERP_MARCH=0",
            "NUFFT_INTERP_MARCH=2", "NUFFT_COARSE_SORT=0", "NUFFT_COARSE_SORT=2", "NUFFT_PREFER_PATCHES=1", "NUFFT_PREFER_RING=0",
            "NUFFT_PRUNED_FFT=0", "NUFFT_COMPACT_DIM1=0")


def _case(t, dims, m, nt=1, ev=0, sm=0, kernel=0, options=""):
    return {"type": t, "dims": list(dims), "m": m, "nt": nt, "ev": ev, "sm": sm, "kernel": kernel, "options": options}


def case_key(c):
    return "%s %s m%d nt%d ev%d sm%d k%d %s" % (c["type"], "x".join(map(str, c["dims"])), c["m"], c["nt"], c["ev"], c["sm"], c["kernel"], c["options"])


def host_matrix():
    cases = []
    for t, _, _ in TYPES:      # main block
        for m in range(2, 11):
            for n in (24, 50, 64, 128, 256):
                for nt in (1, 3):
                    for ev in (0, 1):
                        for sm in (0, 3):
                            cases.append(_case(t, (n, n, n), m, nt, ev, sm))
    for t, _, _ in TYPES:      # switch block
        for m in (2, 4, 7):
            for s in SWITCHES:
                cases.append(_case(t, (128, 128, 128), m, options=s))
            for sm in (1, 2):
                cases.append(_case(t, (128, 128, 128), m, sm=sm))
    for t, _, _ in TYPES:      # small blocks: 1-D and 2-D plans, the other kernels
        for dims in ((64,), (50,), (64, 64), (50, 48)):
            for m in (2, 4, 8):
                cases.append(_case(t, dims, m))
        for kernel in (1, 2, 3):
            cases.append(_case(t, (64, 64, 64), 4, kernel=kernel))
    return cases


def gpu_matrix():
    cases = []
    for n in (50, 64, 128):
        for t, _, _ in TYPES:
            for m in (2, 4, 6, 7):
                for nt in (1, 2):
                    for ev in (0, 1):
                        cases.append(_case(t, (n, n, n), m, nt, ev))
    cases.append(_case("f64r", (128, 128, 128), 4, options="NUFFT_TEST_HALO_ALLOC_FAIL=1"))
    return cases


def _info_fields(L):
    """(name, length) of every integer field of nufft_info, and of the floating-point ones"""
    ints, floats = [], []
    for name, ctype in L.NufftInfo._fields_:
        length = getattr(ctype, "_length_", 1)
        base = ctype._type_ if hasattr(ctype, "_length_") else ctype
        (floats if base is C.c_double else ints).append((name, length))
    return ints, floats


def _flat(value, length):
    return [int(value)] if length == 1 else [int(v) for v in value]


def _create(nufft, c, device):
    L = nufft._lib
    _, dtype, is_complex = next(t for t in TYPES if t[0] == c["type"])
    prm = L.NufftParams()
    prm.struct_size = C.sizeof(L.NufftParams)
    prm.dtype, prm.is_complex, prm.ndim, prm.device = dtype, is_complex, len(c["dims"]), device
    for d, n in enumerate(c["dims"]):
        prm.N[d] = n
    prm.half_support, prm.sigma, prm.kernel, prm.evalmode, prm.ntransforms = c["m"], 2.0, c["kernel"], c["ev"], c["nt"]
    prm.spread_method = c["sm"]
    prm.options = c["options"].encode() if c["options"] else None
    h = C.c_void_p()
    rc = nufft.lib.nufft_plan_create_ex(C.byref(h), C.byref(prm))
    return rc, h


def _record_info(nufft, h):
    L = nufft._lib
    info = L.NufftInfo()
    assert nufft.lib.nufft_plan_info(h, C.byref(info)) == 0
    ints, floats = _info_fields(L)
    rec = {"info": [v for name, n in ints for v in _flat(getattr(info, name), n)],
           "real": [float(v).hex() for name, n in floats for v in ([getattr(info, name)] if n == 1 else getattr(info, name))],
           "options": nufft.lib.nufft_plan_options(h).decode()}
    return rec, info


def _breakdown(nufft, h):
    buf = C.create_string_buffer(4096)
    assert nufft.lib.nufft_workspace_breakdown(h, buf, len(buf)) == 0
    return {k: int(v) for k, v in (item.split("=") for item in buf.value.decode().split(";") if item)}


_POINTS = {}


def _point_sets(nbins):
    """uniform (3 points per bin), folded N(0, 1) of the same size, 24 points per bin — [n][3] Float64 in [0, 2 pi), cached by size"""
    if nbins not in _POINTS:
        _POINTS.clear()      # (one size at a time: the cases are grouped by grid)
        rng = np.random.default_rng(20240607 + nbins)
        two_pi = 2.0 * np.pi
        uniform = rng.random((3, 3 * nbins)) * two_pi
        clustered = np.mod(rng.standard_normal((3, 3 * nbins)), two_pi)
        dense = rng.random((3, 24 * nbins)) * two_pi
        _POINTS[nbins] = (uniform, clustered, dense)
    return _POINTS[nbins]


def _record_point_sets(nufft, h, info, dtype):
    import torch
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    uniform, clustered, dense = _point_sets(int(info.nbins[0]) * int(info.nbins[1]) * int(info.nbins[2]))
    real = torch.float32 if dtype == 0 else torch.float64
    device_sets = {}
    out = []
    for name, pts in (("uniform", uniform), ("clustered", clustered), ("clustered", clustered), ("clustered", clustered), ("dense", dense)):
        if name not in device_sets:
            device_sets[name] = [torch.from_numpy(np.ascontiguousarray(pts[d])).to("cuda", real) for d in range(3)]
        xs = device_sets[name]
        tbl = (C.c_void_p * 3)(*[x.data_ptr() for x in xs])
        rc = nufft.lib.nufft_set_points(h, xs[0].numel(), tbl, stream)
        torch.cuda.synchronize()
        used = []
        for fn in (nufft.lib.nufft_spread_engine_used, nufft.lib.nufft_interp_engine_used, nufft.lib.nufft_sort_columns_used):
            v = C.c_int(-1)
            rc = rc or fn(h, C.byref(v), stream)
            used.append(v.value)
        out.append([rc] + used + [_breakdown(nufft, h).get("sort_scratch", 0)])
    return out


def run(cases, device):
    """{case_key: record}"""
    from nufft_pkg import nufft
    out = {}
    for c in cases:
        rc, h = _create(nufft, c, device)
        if rc != 0:
            out[case_key(c)] = {"rc": rc, "error": nufft.lib.nufft_last_error_message().decode()}
            continue
        rec, info = _record_info(nufft, h)
        rec["rc"] = 0
        if device >= 0:
            rec["workspace_bytes"] = int(info.workspace_bytes)
            rec["breakdown"] = _breakdown(nufft, h)
            rec["sets"] = _record_point_sets(nufft, h, info, info.dtype)
        nufft.lib.nufft_plan_destroy(h)
        out[case_key(c)] = rec
    return out


def num_cus(device):
    import torch
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def snapshot(device):
    from nufft_pkg import nufft
    ints, floats = _info_fields(nufft._lib)
    doc = {"info_fields": [[n, k] for n, k in ints], "real_fields": [[n, k] for n, k in floats]}
    if device >= 0:
        doc["num_cus"] = num_cus(device)
        doc["set_fields"] = ["rc", "spread_engine_used", "interp_engine_used", "sort_columns_used", "sort_scratch_bytes"]
    doc["plans"] = run(gpu_matrix() if device >= 0 else host_matrix(), device)
    return doc


def _names(fields):
    return [n if k == 1 else f"{n}[{i}]" for n, k in fields for i in range(k)]


def flatten(doc, rec):
    """one record as {column: scalar}: the columns of the golden file"""
    out = {"rc": rec["rc"]}
    if rec["rc"] != 0:
        out["error"] = rec["error"]
        return out
    out.update(zip(_names(doc["info_fields"]), rec["info"]))
    out.update(zip(_names(doc["real_fields"]), rec["real"]))
    out["options"] = rec["options"]
    if "sets" in rec:
        out["workspace_bytes"] = rec["workspace_bytes"]
        out.update(("breakdown." + k, v) for k, v in rec["breakdown"].items())
        out.update((f"set{i}.{f}", v) for i, s in enumerate(rec["sets"]) for f, v in zip(doc["set_fields"], s))
    return out


def matrix_digest(keys):
    return hashlib.sha256("\n".join(keys).encode()).hexdigest()


def encode(doc):
    """the golden form: the plans in the matrix's order, column by column, each column run-length encoded as [value, count, value, count, ...]
    (null: the plan has no such field, e.g. a refused one)"""
    flats = [flatten(doc, r) for r in doc["plans"].values()]
    out = {k: v for k, v in doc.items() if k != "plans"}
    out["matrix"] = {"plans": len(flats), "sha256": matrix_digest(list(doc["plans"]))}
    out["columns"] = {}
    for name in dict.fromkeys(k for f in flats for k in f):
        runs = []
        for f in flats:
            v = f.get(name)
            if runs and runs[-2] == v and type(runs[-2]) is type(v):
                runs[-1] += 1
            else:
                runs += [v, 1]
        out["columns"][name] = runs
    return out


def decode(golden):
    """[{column: scalar}] per plan, from the golden form"""
    flats = [{} for _ in range(golden["matrix"]["plans"])]
    for name, runs in golden["columns"].items():
        i = 0
        for v, n in zip(runs[0::2], runs[1::2]):
            for f in flats[i:i + n]:
                if v is not None:
                    f[name] = v
            i += n
        assert i == len(flats), name
    return flats


def write_golden(doc, path):
    enc = encode(doc)
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in enc.items():
            if k != "columns":
                f.write(json.dumps(k) + ": " + json.dumps(v) + ",\n")
        f.write('"columns": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in enc["columns"].items()))
        f.write("\n}}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    doc = snapshot(args.device)
    write_golden(doc, args.out)
    refused = sum(1 for r in doc["plans"].values() if r["rc"] != 0)
    print(f"{len(doc['plans'])} plans ({refused} refused) -> {args.out}")


if __name__ == "__main__":
    main()
