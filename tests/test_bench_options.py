"""CPU tier: what a bench.py run does besides its headline -- nothing without --full, every side measurement with it -- and the side
legs a --full run starts (child processes of their own, stubbed here)."""
import json
import subprocess

import pytest

import bench


def test_plain_run_has_no_side_measurements():
    a = bench.parse_args([])
    assert not a.full and a.extra_scales == "" and a.policy_leg == "" and a.config_legs == "" and a.flag_census == 0 and a.no_cpu_baseline
    assert (a.steps, a.warmup, a.preroll, a.batch, a.level) == (20, 5, 700, 65536, "env")


def test_full_run_has_every_side_measurement():
    a = bench.parse_args(["--full"])
    assert a.full and a.extra_scales == "0.3,0.05" and a.policy_leg == "picking" and a.config_legs == "2,4" and a.flag_census == 20
    assert not a.no_cpu_baseline
    assert bench.parse_args(["--full", "--no-cpu-baseline"]).no_cpu_baseline


def test_side_measurement_options_are_honoured_either_way():
    a = bench.parse_args(["--extra-scales", "0.3", "--flag-census", "5"])
    assert a.extra_scales == "0.3" and a.flag_census == 5 and a.policy_leg == "" and a.config_legs == ""
    a = bench.parse_args(["--full", "--extra-scales", "", "--policy-leg", "", "--config-legs", "", "--flag-census", "0"])
    assert a.extra_scales == "" and a.policy_leg == "" and a.config_legs == "" and a.flag_census == 0


@pytest.fixture
def child_commands(monkeypatch):
    """subprocess.run replaced by a stub that records the command and answers with a minimal side-leg JSON line."""
    cmds = []
    line = {"value": 1.0, "ms_per_step": 1.0, "roofline": {"kernel_ms": 1.0},
            "config": {"done_fraction": 0.0, "mean_rows": 1.0, "heavy_tier_fraction": 0.0, "frame_skip": 50, "envs_per_gpu": 1,
                       "substeps_per_s": 1.0, "launches_per_step": 1.0, "error_flags_or": 0, "flagged_env_steps_per_million": 0.0}}

    def run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps(line) + "\n", stderr="")
    monkeypatch.setattr(bench.subprocess, "run", run)
    bench.LEG_FLAGS.clear()
    return cmds


def test_side_legs_are_full_runs_without_legs_of_their_own(child_commands):
    args = bench.parse_args(["--full"])
    bench.small_action_runs(args)
    bench.policy_run(args)
    bench.config_legs(args)
    assert len(child_commands) == 2 + 1 + 2
    for cmd in child_commands:
        child = bench.parse_args(cmd[2:])
        # (a child keeps the flag census a --full run has: its error flags are reported as side_leg_flags)
        assert child.full and child.no_cpu_baseline and child.flag_census == 20
        assert child.extra_scales == "" and child.policy_leg == "" and child.config_legs == ""
    assert sorted(bench.LEG_FLAGS) == ["action_scale_0.05", "action_scale_0.3", "config2", "config4", "policy_picking"]


def test_plain_run_starts_no_side_legs(child_commands):
    args = bench.parse_args([])
    assert bench.small_action_runs(args) == {} and bench.policy_run(args) is None and bench.config_legs(args) == {}
    assert child_commands == []
