"""my_environment.utils.imitation_kickstarter: the reference's behaviour-cloning kick-start
(``imitationKickstarter.train()`` pre-trains the policy on recorded ``(obs, action)`` pairs with
``imitation``'s ``bc.BC`` before PPO takes over) on ``rl_rocket_amd.bc.bc_train``: the same loss and
``imitation``'s defaults (minibatches of 32, Adam lr 1e-3, ``ent_weight`` 1e-3, ``l2_weight`` 0), on
the device. ``policy`` is an ``rl_rocket_amd.rollout.MlpActorCritic``, or, for demonstrations flown
through ``DiscreteActions3DOF`` (integer actions: indices into its table, from
``RecordTrajectoryCallback`` tuples or from ``obs`` / ``actions`` arrays), an
``rl_rocket_amd.rollout.MlpCategoricalActorCritic``, which is cloned on the indices (an action that is
no integer in ``[0, n_choices)`` raises ``ValueError``); neither ``imitation`` nor
stable-baselines3 is needed. ``play()`` (keyboard control under pygame) is out of scope like
``render()`` and raises.
"""
import numpy as np

BATCH_SIZE, LEARNING_RATE, ENT_WEIGHT, L2_WEIGHT = 32, 1e-3, 1e-3, 0.0  # imitation's bc.BC defaults


def flatten_trajectories(trajectories):
    """``(obs [M, ns], acts [M, na])`` float32 arrays of a list of trajectories, in order: each is a
    tuple ``(obs [L + 1], acts [L], infos, terminal)`` as ``RecordTrajectoryCallback`` builds them,
    or an object with ``.obs`` / ``.acts`` (``imitation``'s ``Trajectory``). The last observation of
    each, on which no action was taken, is dropped."""
    obs, acts = [], []
    for traj in trajectories:
        o, a = (traj[0], traj[1]) if isinstance(traj, (tuple, list)) else (traj.obs, traj.acts)
        o, a = np.asarray(o, dtype=np.float32), np.asarray(a, dtype=np.float32)
        if len(o) != len(a) + 1:
            raise ValueError("a trajectory of %d actions needs %d observations, not %d" % (len(a), len(a) + 1, len(o)))
        obs.append(o[:-1].reshape(len(a), -1))
        acts.append(a.reshape(len(a), -1))
    if not obs:
        raise ValueError("no trajectories")
    return np.concatenate(obs), np.concatenate(acts)


class imitationKickstarter:
    """The reference's constructor and attributes: ``env`` (only ``play()`` would use it), ``obs`` /
    ``actions`` (arrays of pairs), ``policy``, and ``trajectories`` (filled by the caller or by a
    ``RecordTrajectoryCallback``; they take precedence over ``obs`` / ``actions``)."""

    def __init__(self, env=None, obs=None, actions=None, policy=None):
        self.env = env
        self.obs = obs
        self.actions = actions
        self.policy = policy
        self.trajectories = []
        self.optimizer = None  # the Adam of the last train() call
        self.stats = {}        # its last minibatch's figures (rl_rocket_amd.bc.STAT_NAMES)

    def play(self, keys_action_map=None, fps=10):
        raise NotImplementedError("imitationKickstarter.play (gym.utils.play under pygame) is out of scope of "
                                  "rl_rocket_amd; record demonstrations with PolicyEvaluator(record=...)")

    def train(self, n_epochs=1):
        """Pre-train ``self.policy`` on the demonstrations for ``n_epochs`` and return it."""
        import torch

        from rl_rocket_amd.bc import Demonstrations, bc_train

        if self.policy is None:
            raise ValueError("imitationKickstarter.train needs a policy")
        if len(self.trajectories):
            obs, acts = flatten_trajectories(self.trajectories)
        elif self.obs is not None and self.actions is not None:
            obs, acts = self.obs, self.actions
        else:
            raise ValueError("imitationKickstarter.train needs trajectories, or obs and actions")
        dev = next(self.policy.parameters()).device
        demos = Demonstrations.from_arrays(obs, acts, dev)
        self.optimizer = torch.optim.Adam(self.policy.parameters(), lr=LEARNING_RATE, capturable=dev.type == "cuda")
        self.stats = bc_train(self.policy, self.optimizer, demos, n_epochs=n_epochs,
                              batch_size=min(BATCH_SIZE, len(demos)), ent_weight=ENT_WEIGHT, l2_weight=L2_WEIGHT)
        return self.policy


class RecordTrajectoryCallback:
    """The ``callback`` of ``gym.utils.play``: collects the running episode's observations, actions
    and infos and, when it ends, appends ``(obs [L + 1], acts [L], infos, True)`` to
    ``trajectories``."""

    def __init__(self):
        self.trajectories = []
        self.trajectoryObs = []
        self.trajectoryAct = []
        self.trajectoryInfos = []
        self.numTrajectories = 0

    def callback(self, obs_t, obs_tp1, action, rew, done, info):
        self.trajectoryObs.append(obs_t)
        self.trajectoryAct.append(action)
        self.trajectoryInfos.append(info)
        if not done:
            return
        self.trajectoryObs.append(obs_tp1)
        self.trajectories.append((np.array(self.trajectoryObs), np.array(self.trajectoryAct), self.trajectoryInfos, True))
        self.trajectoryObs, self.trajectoryAct, self.trajectoryInfos = [], [], []
        self.numTrajectories += 1

    def returnTrajectories(self):
        """``imitation``'s ``Trajectory`` objects when it is installed, else the tuples themselves
        (``imitationKickstarter.train`` takes either)."""
        for obs, acts, _, _ in self.trajectories:
            if obs.shape[0] != acts.shape[0] + 1:
                raise AssertionError("There needs to be %d observations but there are %d" % (acts.shape[0] + 1,
                                                                                             obs.shape[0]))
        try:
            from imitation.data.types import Trajectory
        except ImportError:
            return list(self.trajectories)
        return [Trajectory(o, a, i, terminal=t) for o, a, i, t in self.trajectories]  # pragma: no cover
