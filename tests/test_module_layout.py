"""rl_rocket_amd.rollout is split by concern (policy.py, learner.py, evaluate.py, bc.py) and stays the
import surface: every name it exported before the split is still its attribute, and is the very
object the new module defines. CPU only."""
import importlib
import os
import subprocess
import sys

# rollout.py's public names before the split, and the underscore names other files import from it
HOMES = {
    "policy": ["MlpActorCritic", "PolicyPack", "POLICY_PRECISIONS", "FOLD_C", "fused_grad_supported",
               "_policy_tensors"],
    "learner": ["PPOGrad", "ClipAdam", "PPOUpdate", "GraphedPPOUpdate", "ppo_update", "clip_adam_supported",
                "_epoch_perms", "_ppo_options", "_train_stats", "_allreduce_grads"],
    "evaluate": ["EvalResult", "PolicyEvaluator", "evaluate_policy", "EVAL_BOUNDS", "EVAL_EVENT", "EVAL_LANDED",
                 "EVAL_NONFINITE", "EVAL_TRUNCATED"],
    "eval_trace": ["EvalTrace", "EpisodeRecord"],
    "bc": ["BCUpdate", "Demonstrations", "bc_train"],
    "rollout": ["DeviceRollout"],
}


def test_rollout_exports_every_name_as_the_object_its_module_defines():
    from rl_rocket_amd import rollout

    assert sum(len(v) for v in HOMES.values()) == 30
    for home, names in HOMES.items():
        mod = importlib.import_module("rl_rocket_amd." + home)
        for name in names:
            assert hasattr(rollout, name), name
            assert getattr(rollout, name) is getattr(mod, name), (home, name)
            if isinstance(getattr(mod, name), type) or callable(getattr(mod, name)):
                assert getattr(mod, name).__module__ == mod.__name__, (home, name)  # defined there, not passed on


def test_bc_imports_without_rollout():
    code = ("import sys, rl_rocket_amd.bc as bc\n"
            "assert 'rl_rocket_amd.rollout' not in sys.modules, 'bc pulled rollout in'\n"
            "assert 'rl_rocket_amd.learner' in sys.modules and 'rl_rocket_amd.policy' in sys.modules\n"
            "from rl_rocket_amd import rollout\n"
            "assert rollout.BCUpdate is bc.BCUpdate\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)  # a fresh child: the import order is its own


def test_lazy_package_attribute_still_resolves_the_evaluator():
    import rl_rocket_amd
    from rl_rocket_amd import evaluate

    assert rl_rocket_amd.PolicyEvaluator is evaluate.PolicyEvaluator
    assert rl_rocket_amd.evaluate_policy is evaluate.evaluate_policy
