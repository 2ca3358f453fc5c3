"""Recorded episodes of the one-launch evaluation (``rr_policy_evaluate_trace``; for a Categorical
policy ``rr_policy_evaluate_discrete_trace``, which adds the plane of chosen indices).

``EvalTrace`` holds the device tensors the recording evaluation writes for the chosen envs;
``EpisodeRecord`` is one of their episodes on the host, with what the reference's env and
``EpisodeAnalyzer`` expose for an episode (rocket_env.py:840-950, wrappers.py:189-235): the state /
action / v_targ / reward dataframes, ``rewards_dict`` per step, the 3D trajectory figures and the
dict the reference passes to ``wandb.log``.
"""
import numpy as np
import torch

from .params import (ACTION_NAMES_3DOF, ACTION_NAMES_6DOF, STATE_NAMES_3DOF, STATE_NAMES_6DOF)

ANALYZER_KEYS = ("ep_history/states", "ep_history/actions", "ep_history/vtarg", "ep_history/rewards",
                 "plots3d/vtarg_trajectory", "plots3d/trajectory", "ep_statistic/landing_success",
                 "ep_statistic/used_mass")  # wrappers.py:216-224, then final_errors/<state name>


class EpisodeRecord:
    """One recorded episode of L steps: ``states`` [L + 1, ns] (row 0 the state it started from, row
    t + 1 the un-reset state after step t: ``SIM.states``), ``actions`` [L, na] (the clipped mean
    actions the env stepped with, normalised), ``terms`` [L, nt] and ``rewards`` [L], float32.
    ``complete`` is False for an episode cut by ``max_steps`` (``partial=True``) or by the
    recording capacity (``clipped=True``); ``length`` is the number of steps the episode took.
    ``choices`` [L] (int32) are the indices of a Categorical policy's choices, whose table rows
    ``actions`` holds; None for a Gaussian policy. Under ``PolicyEvaluator(deterministic=False)`` an action
    row is the clipped SAMPLE the env stepped with (the unclipped sample is not recorded) and ``choices``
    the sampled indices."""

    def __init__(self, cfg, states, actions, terms, rewards, env_id=None, episode=0, length=None, complete=True,
                 choices=None):
        self.cfg = cfg
        self.states = np.asarray(states, dtype=np.float32)
        self.actions = np.asarray(actions, dtype=np.float32)
        self.terms = np.asarray(terms, dtype=np.float32)
        self.rewards = np.asarray(rewards, dtype=np.float32)
        self.choices = None if choices is None else np.asarray(choices, dtype=np.int32)
        self.env_id, self.episode, self.complete = env_id, episode, complete
        self.length = len(self.rewards) if length is None else int(length)
        six = cfg.model == 6
        self.state_names = list(STATE_NAMES_6DOF if six else STATE_NAMES_3DOF)
        self.action_names = list(ACTION_NAMES_6DOF if six else ACTION_NAMES_3DOF)

    def __len__(self):
        return len(self.rewards)

    @property
    def rewards_dict(self):
        """info["rewards_dict"] of every step (what EpisodeAnalyzer collects in rewards_info)."""
        names = self.cfg.term_names
        return [{k: float(row[j]) for j, k in enumerate(names)} for row in self.terms]

    def used_mass(self):
        return self.states[0][-1] - self.states[-1][-1]

    def states_to_dataframe(self):
        import pandas as pd

        return pd.DataFrame(self.states, columns=self.state_names)

    def actions_to_dataframe(self):
        """L + 1 rows like ``SIM.actions``: a zero row, then the denormalised action of every step
        (the shim's ``_denormalize_action``, float32)."""
        import pandas as pd

        from .envs import denormalize_action

        rows = [[0] * len(self.action_names)] + [denormalize_action(self.cfg.model, a) for a in self.actions]
        return pd.DataFrame(rows, columns=self.action_names)

    @property
    def vtarg_history(self):
        """v_targ of every step, computed on the host from the recorded float32 states exactly as
        the shim's ``vtarg_history``. v_0 is the float32 norm of row 0's velocity: the env's v0 only
        when the episode was recorded from its first state (reset before evaluating)."""
        from .envs import compute_vtarg_3dof, compute_vtarg_6dof

        wp = self.cfg.extra["waypoint"]
        if self.cfg.model == 6:
            v_0 = np.linalg.norm(np.asarray(self.states[0][3:6], dtype=np.float32))
            return [compute_vtarg_6dof(s, v_0, wp) for s in self.states[1:]]
        v_0 = np.linalg.norm(self.states[0][3:5])
        return [compute_vtarg_3dof(s, v_0, wp) for s in self.states[1:]]

    def vtarg_to_dataframe(self):
        import pandas as pd

        return pd.DataFrame(self.vtarg_history, columns=["v_x", "v_y", "v_z"] if self.cfg.model == 6 else ["v_x", "v_y"])

    def rewards_to_dataframe(self):
        """pd.DataFrame(rewards_info) of the reference's EpisodeAnalyzer (wrappers.py:207)."""
        import pandas as pd

        return pd.DataFrame(self.terms, columns=list(self.cfg.term_names)).astype(np.float64)

    # -- the reference's episode figures (6DOF: rocket_env.py:861-950) --------------------------------------
    def _six(self):
        if self.cfg.model != 6:
            raise NotImplementedError("the trajectory figures exist for the 6DOF env only (rocket_env.py:861-950)")

    def get_trajectory_plotly(self):
        from .envs import path_figure

        self._six()
        df = self.states_to_dataframe()
        return path_figure(df, (df["vx"], df["vy"], df["vz"]), target_r=self.cfg.extra["landing_radius"])

    def get_vtarg_trajectory(self):
        from .envs import path_figure

        self._six()
        vt = self.vtarg_to_dataframe()
        return path_figure(self.states_to_dataframe(), (vt["v_x"], vt["v_y"], vt["v_z"]), landing_target=[0, 0, 0])

    def get_attitude_trajectory(self):
        from .envs import attitude_figure

        self._six()
        return attitude_figure(self.states_to_dataframe())

    @staticmethod
    def _lines(df):
        """``df.plot()`` under pandas' plotly backend: one line per column over the row index."""
        from .envs import plotly_go

        go = plotly_go()
        return go.Figure(data=[go.Scatter(x=df.index, y=df[c], mode="lines", name=str(c)) for c in df.columns])

    def analyzer_log(self):
        """The dict the reference's EpisodeAnalyzer passes to ``wandb.log`` when an episode ends
        (wrappers.py:216-226), same keys. The history and 3D entries are plotly figures, built here
        if plotly imports (else the dataframes / None); nothing needs wandb."""
        sdf = self.states_to_dataframe()
        frames = {"ep_history/states": sdf, "ep_history/actions": self.actions_to_dataframe(),
                  "ep_history/vtarg": self.vtarg_to_dataframe(), "ep_history/rewards": self.rewards_to_dataframe()}
        try:
            out = {k: self._lines(df) for k, df in frames.items()}
            six = self.cfg.model == 6
            out["plots3d/vtarg_trajectory"] = self.get_vtarg_trajectory() if six else None
            out["plots3d/trajectory"] = self.get_trajectory_plotly() if six else None
        except ImportError:
            out = dict(frames)
            out["plots3d/vtarg_trajectory"] = out["plots3d/trajectory"] = None
        out["ep_statistic/landing_success"] = self.rewards_dict[-1]["rew_goal"]
        out["ep_statistic/used_mass"] = sdf.iloc[0, -1] - sdf.iloc[-1, -1]
        for name, v in zip(self.state_names, np.abs(sdf.iloc[-1, :])):
            out["final_errors/" + name] = v
        return out


class EvalTrace:
    """What one recording evaluation wrote for the K recorded envs, as tensors on the evaluator's
    device (views of its buffers: the next ``run()`` overwrites them):

    ``state`` [K, ne, S + 1, ns], ``action`` [K, ne, S, na], ``terms`` [K, ne, S, nt + 1] (the
    reward terms, then the reward), ``length`` [ne, K] (steps episode k of slot s took; above S where
    the record was clipped) and ``env_ids`` [K] (slot s records env ``env_ids[s]``). ``episodes``
    (the evaluator's [n] count of completed episodes, or None) tells a finished episode from one cut
    by ``max_steps``. ``choice`` [K, ne, S] (int32; None for a Gaussian policy) holds, beside each action
    row of a Categorical policy, the index of the table row it is. Rows past an episode's length are not
    written."""

    def __init__(self, cfg, state, action, terms, length, env_ids, episodes=None, choice=None):
        self.cfg, self.state, self.action, self.terms, self.length = cfg, state, action, terms, length
        self.env_ids, self.episodes, self.choice = env_ids, episodes, choice
        self._slot = {int(e): s for s, e in enumerate(torch.as_tensor(env_ids).cpu().tolist())}

    @property
    def steps(self):
        return self.action.shape[2]

    def episode(self, env_id, k=0, partial=False, clipped=False):
        """Episode ``k`` of env ``env_id`` as an ``EpisodeRecord`` on the host (one synchronise).
        Raises for an episode that did not finish within ``max_steps`` unless ``partial=True`` and
        for one longer than the recording capacity unless ``clipped=True`` (the record is then cut
        at the capacity)."""
        if int(env_id) not in self._slot:
            raise KeyError("env %d was not recorded (record=%s)" % (env_id, sorted(self._slot)))
        s = self._slot[int(env_id)]
        ne = self.length.shape[0]
        if not 0 <= k < ne:
            raise IndexError("episode %d of %d" % (k, ne))
        cap = self.steps
        done = ne if self.episodes is None else self.episodes[int(env_id)]
        # one device-to-host copy: the length, the episodes count and the episode's rows
        flat = torch.cat([self.length[k, s].reshape(1).float(), torch.as_tensor(done, device=self.length.device)
                          .reshape(1).float(), self.state[s, k].reshape(-1), self.action[s, k].reshape(-1),
                          self.terms[s, k].reshape(-1)] +
                         ([] if self.choice is None else [self.choice[s, k].float()])).cpu().numpy()  # < 2^24: exact
        length, done = int(flat[0]), int(flat[1])
        if k > done or (k == done and not partial):
            raise ValueError("env %d did not finish episode %d within max_steps (%d finished)%s" % (
                env_id, k, done, "" if k > done else "; partial=True returns the steps it took"))
        if length > cap and not clipped:
            raise ValueError("episode %d of env %d took %d steps, the record holds %d (record_steps); "
                             "clipped=True returns the first %d" % (k, env_id, length, cap, cap))
        n = min(length, cap)
        ns, na, nt1 = self.state.shape[-1], self.action.shape[-1], self.terms.shape[-1]
        o = 2
        st = flat[o:o + (cap + 1) * ns].reshape(cap + 1, ns)[:n + 1]
        o += (cap + 1) * ns
        ac = flat[o:o + cap * na].reshape(cap, na)[:n]
        o += cap * na
        tm = flat[o:o + cap * nt1].reshape(cap, nt1)[:n]
        o += cap * nt1
        ch = None if self.choice is None else flat[o:o + cap][:n].astype(np.int32)
        return EpisodeRecord(self.cfg, st.copy(), ac.copy(), tm[:, :-1].copy(), tm[:, -1].copy(), env_id=int(env_id),
                             episode=k, length=length, complete=(k < done and length <= cap), choices=ch)
