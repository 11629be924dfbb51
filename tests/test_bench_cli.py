"""bench.py command-line contract that can be checked without a GPU: `--gpus N` must never silently run fewer
ranks than it reports (`bench.py --gpus 8` used to print n_gpus = 1)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def test_gpus_flag_refuses_to_run_with_fewer_visible_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("needs a box with fewer than 2 GPUs")
    r = _run(["--gpus", "2"])
    assert r.returncode != 0
    assert "only" in r.stderr and "GPU(s) visible" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_gpus_flag_must_match_world_size():
    r = _run(["--gpus", "4"], {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
    assert '"n_gpus"' not in r.stdout


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_config_leads_with_the_other_baseline_configurations():
    """The driver's parser keeps the first 20 scalar keys of `config`.  Round 5 pushed the C3 / C4 values behind stage times and
    sort keys and they fell out of the driver-observed line: whatever else `config` carries, and in whatever
    order it was assembled, the lead keys come first."""
    b = _load_bench()
    want = ("workload", "direct_value", "fast_value", "type2_value", "c3_value", "c3_type2_value", "c3_spread_ms", "c3_interp_ms",
            "c3_set_points_ms", "c3_fp32_frac", "c3_direct_value", "c4_value", "c4_type2_value", "c4_spread_ms", "c4_interp_ms",
            "c4_direct_value", "refproto_f64_type1_value", "refproto_f64_type2_value", "refproto_c128_type1_value", "workspace_bytes")
    assert tuple(b.CONFIG_LEAD_KEYS) == want and len(want) == 20
    # a config assembled as main() does it: workload / protocol / engine / lists / stage times first, the flattened records last
    cfg = {"workload": "C2 ...", "protocol": "p", "spread_engine": "marching_ring", "spread_tile": [1, 2, 3], "ring_column": [32, 32],
           "ring_segments": 1, "ring_halo": 1, "workspace_bytes": 1, "sort_columns": True, "sort_method": "column_layers",
           "set_points_ms": 0.5, "spread_ms": 2.0, "fft_ms": 0.7, "deconv_ms": 0.1, "interp_ms": 1.2, "type2_value": 4e9, "parallelism": "x",
           "direct_value": 3e9, "direct_ms_per_step": 3.3, "fast_value": 3.1e9, "fast_ms_per_step": 3.2, "fast_type2_value": 4.3e9,
           "other_configs": {"c3": {}, "c4": {}}}
    for name in ("c4", "c3"):
        for k in ("value", "ms_per_step", "type2_value", "type2_ms_per_step", "spread_ms", "interp_ms", "spread_engine", "roofline_frac",
                  "set_points_ms", "direct_value", "fp32_frac"):
            cfg[f"{name}_{k}"] = 1.0
    cfg["refproto_c128_type1_value"] = cfg["refproto_c128_type2_value"] = cfg["refproto_f64_type1_value"] = cfg["refproto_f64_type2_value"] = 1.0
    led = b.lead_config(cfg)
    assert set(led) == set(cfg) and all(led[k] == cfg[k] for k in cfg)          # nothing lost, nothing changed
    kept = b.first_scalar_keys(led, 20)
    missing = [k for k in want if k not in kept and k != "c4_fp32_frac"]
    assert not missing, missing
    assert kept[0] == "workload"
    # what main() itself emits goes through lead_config
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'result["config"] = lead_config(result["config"])' in src
    flat = src[src.index("for name, r in others.items():"):]
    for k in ("value", "type2_value", "spread_ms", "interp_ms", "set_points_ms", "fp32_frac", "direct_value"):
        assert f'"{k}"' in flat[:1500], k


def test_profile_lookup_is_window_mode_aware():
    """`roofline.interp` used to quote the polynomial instantiation's profile under the Direct() headline."""
    b = _load_bench()
    d = [os.path.basename(f) for f in b.profile_files("c2", "_traffic.json", "Direct")]
    p = [os.path.basename(f) for f in b.profile_files("c2", "_traffic.json", "FastApproximation")]
    assert d and p and not set(d) & set(p)
    assert all("_c2_direct_" in f for f in d) and not any("_direct" in f for f in p)
    assert not any("_c3_" in f or "_c4_" in f for f in d + p)
    t, src, us = b.pmc_traffic("interp_march_staged_kernel<double, false, 4, false>", "c2", "Direct")
    assert t and "_c2_direct_" in src and us
    t2, src2, us2 = b.pmc_traffic("interp_march_staged_kernel<double, false, 4, true>", "c2", "FastApproximation")
    assert t2 and "_direct" not in src2 and us2 and us2 != us
    assert b.pmc_traffic("interp_march_staged_kernel<double, false, 4, true>", "c2", "Direct")[0] is None
    sq = b.sq_counters("interp_march_staged_kernel<double, false, 4, false>", "c2", "Direct")
    assert sq is None or "_c2_direct_" in sq["source"]


def test_full_and_dump_outputs_are_options():
    """A plain run times the headline only; what else the benchmark measures sits behind --full, and --dump-outputs DIR writes
    the last timed step's outputs."""
    r = _run(["--help"])
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "full = world == 1 and a.full and not a.only_headline" in src
    assert "type2=a.full" in src


def test_output_sample_is_fixed_and_bounded():
    """--dump-outputs: the same coefficients on every run (indices seeded, depending on the shape only), all of them when they
    fit, at most DUMP_SAMPLE over all components (64 MB in complex128 at the most), (re, im) in the spectrum's precision."""
    import numpy as np
    import torch
    b = _load_bench()
    assert b.DUMP_SAMPLE * 16 <= 64 * 2 ** 20
    g = torch.Generator().manual_seed(1)
    outs = tuple(torch.randn(40, 32, 9, dtype=torch.complex128, generator=g) for _ in range(3))
    b.DUMP_SAMPLE = 3 * 1000
    s1, s2 = b.output_sample(outs), b.output_sample(tuple(o.clone() for o in outs))
    assert sorted(s1) == ["type1_uhat_c0", "type1_uhat_c1", "type1_uhat_c2"]
    for name, arr in s1.items():
        assert arr.dtype == np.float64 and arr.ndim == 2 and arr.shape[1] == 2 and 900 < arr.shape[0] <= 1000
        assert np.array_equal(arr, s2[name])
    # the sampled coefficients are the ones at the seeded flat indices
    idx = np.unique(np.random.default_rng(0).integers(0, outs[0].numel(), 1000))
    assert np.array_equal(s1["type1_uhat_c1"], torch.view_as_real(outs[1].reshape(-1)).numpy()[idx])
    # small spectra are written whole; complex64 spectra as float32
    small = (torch.randn(4, 5, 3, dtype=torch.complex64, generator=g),)
    whole = b.output_sample(small)["type1_uhat_c0"]
    assert whole.dtype == np.float32 and np.array_equal(whole, torch.view_as_real(small[0].reshape(-1)).numpy())
