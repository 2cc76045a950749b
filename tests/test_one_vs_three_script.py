"""BASELINE configs[0] from a script: a driver subprocess set up by INTEGRATION.md §1's recipe — repo root and compat/ first on
PYTHONPATH, `torch.utils.tensorboard` (compat/tensorboard), the config.toml through `toml` (compat/toml), `from libriichi.arena
import OneVsThree` (this repository's package) with a log_dir, 8 hanchan (games_per_iter = 8) — and its printed rankings are
compared with the reference-shaped oracle loop driven by the same two engines.  The subprocess has no GPU: a test-side
sitecustomize (tests/host/sitecustomize_emu) points the arena at the host emulator build of the same kernels.

The two engines are the reference's MortalEngine over tiny random-init checkpoints (seeds 1 and 2), recorded by
tests/golden/record_reference_engines.py (tests/golden/reference_*, case `cfg0`) and replayed by tests/recorded_engine.RecordedEngine:
a decision whose obs or mask differs from what the reference engine saw fails the test.  MORTAL_AMD_CFG0_REAL=1: the same
against the REAL library (no emulator injection, libmortal_amd.so on cuda:0)."""
import os
import json
import subprocess
import sys

REAL = os.environ.get("MORTAL_AMD_CFG0_REAL") == "1"  # the real libmortal_amd.so on cuda:0 instead of the host emulator
KEY = 0x55DFAA4CEF265CD7  # a TOML integer is a signed 64-bit value (config.toml: seed_key)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")

VERSION = 4


def _driver(cfg_path):
    """The subprocess: the config through compat/toml, the recorded engines, one OneVsThree.py_vs_py with a log_dir."""
    import torch.utils.tensorboard  # noqa: F401  (compat/tensorboard)
    import toml

    import recorded_engine as R
    from libriichi.arena import OneVsThree

    with open(cfg_path, encoding="utf-8") as f:
        cfg = toml.load(f)["1v3"]
    chal, cham = (R.RecordedEngine(R.decisions("cfg0", who), VERSION, cfg[who]["name"]) for who in R.ENGINES)
    env = OneVsThree(disable_progress_bar=True, log_dir=cfg["log_dir"])
    rankings = env.py_vs_py(challenger=chal, champion=cham, seed_start=(10000, cfg["seed_key"]), seed_count=cfg["games_per_iter"] // 4)
    print("rankings " + json.dumps([int(x) for x in rankings]))


def test_one_vs_three_script_runs_unchanged(oracle, tmp_path):
    import recorded_engine as R
    import test_reference_engine as T
    from mortal_amd.pool import default_deal_algo

    cfg = tmp_path / "config.toml"
    cfg.write_text(f"""
[1v3]
seed_key = {KEY}
games_per_iter = 8
iters = 1
log_dir = '{tmp_path / "logs"}'

[1v3.champion]
name = 'champion'

[1v3.challenger]
name = 'challenger'

[1v3.akochan]
enabled = false
""")
    # repo root and compat/ before anything else on PYTHONPATH; + the test-only emulator injection
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "compat")] + ([] if REAL else [os.path.join(HOST, "sitecustomize_emu")])),
               OMP_NUM_THREADS="4")
    if REAL:
        env.pop("MORTAL_AMD_TEST_EMU", None)
    else:
        env["MORTAL_AMD_TEST_EMU"] = "1"
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_one_vs_three_script as S; S._driver({str(cfg)!r})"
    run = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, stdin=subprocess.DEVNULL,
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    m = [ln for ln in run.stdout.splitlines() if ln.startswith("rankings ")]
    assert m, run.stdout[-2000:]
    got = json.loads(m[-1][len("rankings "):])
    assert sum(got) == 8

    # the same two engines on the oracle loop (arena/game.rs:286-304), and the rankings the reference engines reached there
    chal, cham = (R.RecordedEngine(R.decisions("cfg0", who), VERSION, who) for who in R.ENGINES)
    want = T._oracle_rankings(oracle, chal, cham, (10000, KEY), 2, VERSION, default_deal_algo())
    assert got == want == R.fixture()["one_vs_three"]["cfg0"]["rankings"], (got, want, run.stdout[-500:])
    print(f"cfg0 ({'libmortal_amd.so' if REAL else 'host emulator'}): challenger rankings {got} == oracle loop {want}; script stdout tail: {run.stdout[-300:]!r}")
    # log_dir side effect (one_vs_three.rs:127-129,195-225): one gzip'd mjai log per hanchan
    logs = sorted(os.listdir(tmp_path / "logs"))
    assert len(logs) == 8 and all(f.endswith(".json.gz") for f in logs), logs
