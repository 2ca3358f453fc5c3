"""my_environment.wrappers: ``RewardAnnealing`` (reference wrappers.py:68-86),
``EpisodeAnalyzer`` (wrappers.py:189-235, the wrapper main_6DOF.make_eval_env puts around the
evaluation env) and ``DiscreteActions3DOF`` (wrappers.py:24-35, the ``Discrete(4)`` action space
sensitivity_test.py evaluates a PPO model behind) restated over the shims. The other plotting / video
wrappers (EpisodeAnalyzer6DOF, RecordVideoFigure: gym RecordVideo + pyvista rendering;
GaudetStateObs: never used by the training drivers) are out of scope and raise.

For vectorised training use ``rl_rocket_amd.RocketVecEnv(..., reward_annealing=True)``,
which computes the annealed reward inside the step kernel, and for the discrete actions on the
device ``rl_rocket_amd.rollout.MlpCategoricalActorCritic`` with a ``RocketBatch``.
"""
import numpy as np

from rl_rocket_amd.envs import Rocket6DOF
from rl_rocket_amd.gym_compat import HAVE_GYM, Discrete
from rl_rocket_amd.params import DISCRETE_TABLE_3DOF

if HAVE_GYM:  # pragma: no cover
    import gym

    _Base = gym.Wrapper
else:
    class _Base:
        def __init__(self, env):
            self.env = env
            self.action_space = env.action_space
            self.observation_space = env.observation_space

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)
            return getattr(self.env, name)

        @property
        def unwrapped(self):
            return getattr(self.env, "unwrapped", self.env)

        def reset(self, **kw):
            return self.env.reset(**kw)

        def step(self, action):
            return self.env.step(action)


class RewardAnnealing(_Base):
    """reward = attitude_constraint + rew_goal - xi * (a_thrust + 1) (wrappers.py:72-86)."""

    def __init__(self, env, thrust_penalty: float = 0.01):
        super().__init__(env)
        self.xi = self.reward_coefficients.get("xi", thrust_penalty)

    def step(self, action):
        obs, _, done, info = self.env.step(action)
        old = info["rewards_dict"]
        rewards_dict = {k: old[k] for k in ("attitude_constraint", "rew_goal")}
        a_t = action[2] if isinstance(self.unwrapped, Rocket6DOF) else action[1]
        rewards_dict["thrust_penalty"] = -self.xi * (a_t + 1)
        info["rewards_dict"] = rewards_dict
        return obs, sum(rewards_dict.values()), done, info


class DiscreteActions3DOF(_Base):
    """The 3DOF env behind a ``Discrete(len(disc_to_cont))`` action space (wrappers.py:24-35): choice
    ``i`` steps the env with row ``i`` of the table, a [gimbal, thrust] pair. The default table is the
    reference's: engine off, full thrust gimballed left, straight, right."""

    def __init__(self, env, disc_to_cont=DISCRETE_TABLE_3DOF):
        super().__init__(env)
        self.disc_to_cont = [list(row) for row in disc_to_cont]
        space = Discrete(len(self.disc_to_cont))
        self.action_space = space.to_gym()

    def action(self, act):
        return np.asarray(self.disc_to_cont[int(act)])

    def step(self, act):
        return self.env.step(self.action(act))

    def get_keys_to_action(self):
        raise NotImplementedError("get_keys_to_action (pygame keyboard play) is out of scope of rl_rocket_amd")


class EpisodeAnalyzer(_Base):
    """Per-episode analysis of a single Rocket6DOF env (wrappers.py:189-235): keeps every step's
    ``info["rewards_dict"]``; when the episode ends it builds the states / actions / v_targ
    dataframes (pandas) and the episode statistics the reference logs — final absolute state
    errors per state name, landing success (the last ``rew_goal``), used mass — and, when a
    wandb run is active, logs them with the reference's plots (plotly / matplotlib, imported
    only then). Without a wandb run the reference calls ``fig.show()`` (a browser window); here
    the statistics are kept in ``last_episode`` and the figure is built on request
    (``env.unwrapped.get_trajectory_plotly()``), so headless evaluation does not block."""

    def __init__(self, env):
        super().__init__(env)
        assert isinstance(env.unwrapped, Rocket6DOF)
        self.rewards_info = []
        self.last_episode = None

    def step(self, action):
        obs, rew, done, info = self.env.step(action)
        self.rewards_info.append(info["rewards_dict"])
        if done:
            u = self.env.unwrapped
            states = u.states_to_dataframe()
            stats = {"final_errors/" + k: v for k, v in zip(u.state_names, np.abs(states.iloc[-1, :]))}
            stats["ep_statistic/landing_success"] = info["rewards_dict"]["rew_goal"]
            stats["ep_statistic/used_mass"] = states.iloc[0, -1] - states.iloc[-1, -1]
            self.last_episode = {"stats": stats, "states": states, "actions": u.actions_to_dataframe(),
                                 "vtarg": u.vtarg_to_dataframe(), "rewards": list(self.rewards_info)}
            run = _wandb_run()
            if run is not None:  # pragma: no cover - wandb is not installed in this image
                import matplotlib.pyplot as plt
                import pandas as pd

                import wandb

                fig_rew = pd.DataFrame(self.rewards_info).plot()
                plt.close()
                wandb.log({"ep_history/states": states.plot(),
                           "ep_history/actions": self.last_episode["actions"].plot(),
                           "ep_history/vtarg": self.last_episode["vtarg"].plot(),
                           "ep_history/rewards": fig_rew,
                           "plots3d/vtarg_trajectory": u.get_vtarg_trajectory(),
                           "plots3d/trajectory": u.get_trajectory_plotly(),
                           **stats})
            self.rewards_info = []
        return obs, rew, done, info


def _wandb_run():
    try:
        import wandb
    except ImportError:
        return None
    return wandb.run


def _out_of_scope(name):
    def _raise(*a, **k):
        raise NotImplementedError("%s (wandb / plotly / pygame visualisation) is out of scope of rl_rocket_amd" % name)
    return _raise


EpisodeAnalyzer6DOF = _out_of_scope("EpisodeAnalyzer6DOF")
RecordVideoFigure = _out_of_scope("RecordVideoFigure")
GaudetStateObs = _out_of_scope("GaudetStateObs")

__all__ = ["RewardAnnealing", "EpisodeAnalyzer", "EpisodeAnalyzer6DOF", "RecordVideoFigure", "GaudetStateObs",
           "DiscreteActions3DOF"]
