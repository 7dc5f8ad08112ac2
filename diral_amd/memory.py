"""Replay memory on the device: the DRQN agent's ``Memory`` (utils/memory.py:162-194) for B envs at once.

The reference's slot loop ends with ``memory.add((state, action, reward, next_state))`` and its training step begins with
``Memory.sample(batch_size, step_size)`` followed by ``DRQN.get_states_user`` and the three like it
(algorithms/drl_drqn.py:294-377), which regroup the windows user-major into ``[num_users * batch, step_size, S]``.
:class:`ReplayMemory` keeps three rings of ``capacity + 1`` rows in device memory - torch owns them -, writes K slots of a
K-slot launch into them with ONE launch of ``diral_memory_add`` and answers ``sample`` with ONE launch of
``diral_memory_sample`` (include/diral_env.h) that already leaves the regrouped layout.  The driver always has
``state = next_state``, so a state is stored once; `begin` starts a new trajectory (and empties the memory).  The sampled
windows are distinct (env, start) pairs - ``np.random.choice(replace=False)``'s guarantee - from a keyed permutation of
(seed, call number), not NumPy's stream; they can also be injected.  No network, no TD target, no optimiser.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._tensors import MSG_OUT, _ptr, check_tensor, dtype_code, policy_seed
from .config import DT_BF16, DT_F16, DT_F32, DT_F64, DiralMemory, DiralMemoryAdd, DiralMemorySample
from .vec_env import check_status

RING_DTYPES = {torch.float32: DT_F32, torch.float64: DT_F64}
OUT_DTYPES = {torch.float32: DT_F32, torch.float64: DT_F64, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
OUT_KEYS = ("states", "actions", "rewards", "next_states")


class ReplayMemory:
    """``capacity`` is the reference's ``max_size``; ``dtype`` the rings' (float32 or float64).  `count_on_device`: the
    number of transitions lives in an int64 device tensor (`count_dev`) that every `add` moves on with a one-thread
    launch, so that a captured [add, sample_clocked] pair moves on at every replay; ``len()`` then synchronises."""

    def __init__(self, capacity: int, batch: int, num_users: int, state_space: int, dtype: torch.dtype = torch.float32,
                 seed: int = 0, device="cuda:0", count_on_device: bool = False, env_offset: int = 0):
        if dtype not in RING_DTYPES:
            raise ValueError("dtype must be torch.float32 or torch.float64")
        if min(int(capacity), int(batch), int(num_users), int(state_space)) < 1:
            raise ValueError("capacity, batch, num_users and state_space must be >= 1")
        self.lib = _lib.load()
        self.C, self.B, self.N, self.S = int(capacity), int(batch), int(num_users), int(state_space)
        self.dtype, self.device = dtype, torch.device(device)
        self.seed = policy_seed(seed, env_offset)         # shards of a batch keep their own memory and draw other windows
        rows = self.C + 1
        self.states = torch.zeros((rows, self.B, self.N, self.S), dtype=dtype, device=self.device)
        self.actions = torch.zeros((rows, self.B, self.N), dtype=torch.int32, device=self.device)
        self.rewards = torch.zeros((rows, self.B, self.N), dtype=dtype, device=self.device)
        self.count = 0                                    # transitions added so far (host form)
        self.count_dev = torch.zeros((1,), dtype=torch.int64, device=self.device) if count_on_device else None
        self.bad_samples = torch.zeros((1,), dtype=torch.int32, device=self.device)   # windows answered with zeros
        self.last_idx: Optional[torch.Tensor] = None      # the windows of the last sample: feed them back as idx= / env=
        self.last_env: Optional[torch.Tensor] = None
        self._state0: Optional[torch.Tensor] = None
        self._t = 0                                       # sample call number `k` draws with policy_seed(seed, k)
        self._keep: tuple = ()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _desc(self) -> DiralMemory:
        m = DiralMemory()
        m.struct_bytes = ctypes.sizeof(DiralMemory)
        m.capacity, m.batch, m.num_users, m.state_space, m.dtype = self.C, self.B, self.N, self.S, RING_DTYPES[self.dtype]
        m.states, m.actions, m.rewards = _ptr(self.states), _ptr(self.actions), _ptr(self.rewards)
        m.count, m.count_dev = self.count, _ptr(self.count_dev)
        return m

    def __len__(self) -> int:
        return min(self.count if self.count_dev is None else int(self.count_dev.item()), self.C)

    # ---- writing ----
    def begin(self, state: torch.Tensor) -> None:
        """Start a trajectory at `state` [B, N, S] (the bootstrap's, main_test.py:89-94): the memory is emptied, and the
        next `add` stores `state` in front of its own - it is read then, not now, and must stay as it is until then."""
        self._float("state", state, (self.B, self.N, self.S))
        self._state0 = state
        self.count = 0
        if self.count_dev is not None:
            self.count_dev.zero_()

    def _float(self, name: str, t, shape: tuple) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype not in RING_DTYPES:
            raise ValueError("%s must be a float32 or float64 tensor %s" % (name, list(shape)))
        check_tensor(name, t, t.dtype, shape, self.device, MSG_OUT)

    def add_many(self, actions: torch.Tensor, rewards: torch.Tensor, states: torch.Tensor) -> None:
        """K transitions in one launch: ``actions`` [K, B, N] int32, ``rewards`` [K, B, N] or one [B, N] row stored for
        every slot, ``states`` [K, B, N, S] - the NEXT state of every slot (float32 or float64, converted to the rings'
        dtype).  K <= capacity."""
        if not isinstance(actions, torch.Tensor) or actions.dim() != 3:
            raise ValueError("actions must be an int32 tensor [K, B, N]")
        K = int(actions.shape[0])
        if K < 1 or K > self.C:
            raise ValueError("add_many: 1 <= K <= capacity (%d), got %d" % (self.C, K))
        if self.count == 0 and self.count_dev is None and self._state0 is None:
            raise ValueError("add before begin(state)")
        check_tensor("actions", actions, torch.int32, (K, self.B, self.N), self.device)
        self._float("states", states, (K, self.B, self.N, self.S))
        bcast = isinstance(rewards, torch.Tensor) and rewards.dim() == 2
        self._float("rewards", rewards, (self.B, self.N) if bcast else (K, self.B, self.N))
        s0 = self._state0
        if s0 is not None and s0.dtype != states.dtype:
            s0 = s0.to(states.dtype)
        a = DiralMemoryAdd()
        a.struct_bytes = ctypes.sizeof(DiralMemoryAdd)
        a.slots, a.next_states, a.state0, a.src_dtype = K, _ptr(states), _ptr(s0), dtype_code(states)
        a.actions, a.rewards, a.rewards_dtype, a.rewards_broadcast = _ptr(actions), _ptr(rewards), dtype_code(rewards), int(bcast)
        m = self._desc()
        check_status(self.lib.diral_memory_add(ctypes.byref(m), ctypes.byref(a), self._stream()), "diral_memory_add")
        self._keep = (actions, rewards, states, s0)
        self._state0 = None
        if self.count_dev is None:
            self.count += K
        else:
            check_status(self.lib.diral_clock_add(ctypes.c_void_p(_ptr(self.count_dev)), K, self._stream()), "diral_clock_add")

    def add(self, action: torch.Tensor, reward: torch.Tensor, next_state: torch.Tensor) -> None:
        """``memory.add((state, action, reward, next_state))`` of every env: [B, N], [B, N], [B, N, S]."""
        self.add_many(action.unsqueeze(0), reward.unsqueeze(0), next_state.unsqueeze(0))

    def add_rollout(self, actions_seq: torch.Tensor, out: Dict[str, Optional[torch.Tensor]]) -> None:
        """The K slots of ``VecV2VEnv.rollout`` / ``DriverLoop.rollout(actions_seq, ..., states="all")``: `out` is the
        dict it returned; the rewards stored are its ``shaped`` ones (what the driver hands to memory.add)."""
        st = out.get("states")
        if st is None or st.dim() != 4:
            raise ValueError("add_rollout needs the rollout's states='all' output [K, B, N, S]")
        self.add_many(actions_seq, out["shaped"], st)

    def add_prefill(self, states: torch.Tensor, actions: torch.Tensor, rews0: torch.Tensor) -> None:
        """What ``DriverLoop.prefill`` returned, stored with the stale bootstrap rewards `rews0` [B, N] for every slot
        (main_test.py:110-112)."""
        self.add_many(actions, rews0, states)

    # ---- a launch that writes the ring rows itself (VecV2VEnv.rollout / prefill with memory=) ----
    def ring_block(self, K: int, batch: int, num_users: int, state_space: int, dtype: torch.dtype, device,
                   where: str = "memory") -> DiralMemory:
        """The descriptor a K-slot launch writes its transitions through (`diral_env_rollout_memory` /
        `diral_env_prefill_memory`): slot k's state vector goes to state row ``count + 1 + k``, its actions and reward
        to row ``count + k``, mod ``capacity + 1`` - `add_many`'s rows, without the scratch and without its launch.
        Checks K and the launch's shapes, dtype and device against the rings; nothing is written or moved on here -
        `commit` does that behind a launch that was taken."""
        K = int(K)
        if K < 1 or K > self.C:
            raise ValueError("%s: 1 <= K <= capacity (%d), got %d" % (where, self.C, K))
        if (int(batch), int(num_users), int(state_space)) != (self.B, self.N, self.S):
            raise ValueError("%s: the memory holds [B=%d, N=%d, S=%d] rows, the launch writes [%d, %d, %d]"
                             % (where, self.B, self.N, self.S, batch, num_users, state_space))
        if dtype != self.dtype:
            raise ValueError("%s: the rings are %s, the launch writes %s (no conversion: use add_rollout / add_prefill)"
                             % (where, self.dtype, dtype))
        if torch.device(device) != self.device:
            raise ValueError("%s: the memory lives on %s, the env on %s" % (where, self.device, device))
        if self.count == 0 and self.count_dev is None and self._state0 is None:
            raise ValueError("add before begin(state)")
        return self._desc()

    def commit(self, K: int) -> Optional[torch.Tensor]:
        """Behind a launch that wrote K transitions through `ring_block`: the pending `begin` state goes to state row
        `count` (a stream-ordered copy, cast to the rings' dtype - the launch neither reads nor writes that row), the
        count moves on by K.  Returns a view of the last state row written, or None when the count lives on the device."""
        if self._state0 is not None:
            self.states[self.count % (self.C + 1)].copy_(self._state0)   # (a begin has zeroed both counts: row 0)
            self._state0 = None
        if self.count_dev is None:
            self.count += int(K)
            return self.states[self.count % (self.C + 1)]
        check_status(self.lib.diral_clock_add(ctypes.c_void_p(_ptr(self.count_dev)), int(K), self._stream()), "diral_clock_add")
        return None

    # ---- reading ----
    def _sample(self, M: int, step: int, out_dtype, idx, env, last_only, out, seed, clock, offset):
        M, step = int(M), int(step)
        out_dtype = self.dtype if out_dtype is None else out_dtype
        if out_dtype not in OUT_DTYPES:
            raise ValueError("out_dtype must be a torch float dtype")
        if M < 1 or step < 1:
            raise ValueError("batch_size and step_size must be >= 1")
        rows = self.N * M
        shapes = dict(states=((rows, step, self.S), out_dtype), next_states=((rows, step, self.S), out_dtype),
                      actions=((rows,) if last_only else (rows, step), torch.int32),
                      rewards=((rows,) if last_only else (rows, step), self.dtype))
        res = {}
        for k in OUT_KEYS:
            shape, dt = shapes[k]
            if out is None:
                res[k] = torch.empty(shape, dtype=dt, device=self.device)
            else:
                res[k] = out.get(k)
                if res[k] is not None:
                    check_tensor("out[%r]" % k, res[k], dt, shape, self.device, MSG_OUT)
        if (idx is None) != (env is None):
            raise ValueError("idx and env come together")
        if idx is not None:
            idx = torch.as_tensor(idx, dtype=torch.int32, device=self.device).reshape(M).contiguous()
            env = torch.as_tensor(env, dtype=torch.int32, device=self.device).reshape(M).contiguous()
        idx_out = torch.empty((M,), dtype=torch.int32, device=self.device)
        env_out = torch.empty((M,), dtype=torch.int32, device=self.device)
        s = DiralMemorySample()
        s.struct_bytes = ctypes.sizeof(DiralMemorySample)
        s.windows, s.step, s.out_dtype, s.last_only = M, step, OUT_DTYPES[out_dtype], int(bool(last_only))
        s.idx, s.env, s.seed, s.clock, s.clock_offset = _ptr(idx), _ptr(env), seed, _ptr(clock), int(offset)
        s.states_out, s.next_states_out = _ptr(res["states"]), _ptr(res["next_states"])
        s.actions_out, s.rewards_out = _ptr(res["actions"]), _ptr(res["rewards"])
        s.idx_out, s.env_out, s.bad_samples = _ptr(idx_out), _ptr(env_out), _ptr(self.bad_samples)
        m = self._desc()
        check_status(self.lib.diral_memory_sample(ctypes.byref(m), ctypes.byref(s), self._stream()), "diral_memory_sample")
        self._keep = (idx, env, clock, res)
        self.last_idx, self.last_env = idx_out, env_out
        return res["states"], res["actions"], res["rewards"], res["next_states"]

    def sample(self, batch_size: int, step_size: int, out_dtype: Optional[torch.dtype] = None, idx=None, env=None,
               last_only: bool = False, out: Optional[Dict[str, torch.Tensor]] = None
               ) -> Tuple[Optional[torch.Tensor], ...]:
        """``batch = memory.sample(batch_size, step_size)`` + the four ``get_*_user`` + the reshapes of ``train``
        (drl_drqn.py:211-243): returns ``(states, actions, rewards, next_states)`` with shapes
        ``[N * batch_size, step_size, S]``, ``[N * batch_size, step_size]`` (int32), the same (rings' dtype), and the
        states' - row ``n * batch_size + m``.  `out_dtype`: the two state outputs' (float32 rings: float32 / float16 /
        bfloat16; float64 rings: float64 / float32).  `last_only`: actions and rewards ``[N * batch_size]``, the last
        step's.  `idx` / `env` [batch_size] int32: the windows given instead of drawn (start in ``[0, len - step_size)``,
        env in ``[0, B)``; anything else gives zeros and counts in `bad_samples`).  `out`: a dict of caller-owned output
        tensors by name; a name it leaves out is not produced (returned as None).  `last_idx` / `last_env` hold the
        windows of the call."""
        r = self._sample(batch_size, step_size, out_dtype, idx, env, last_only, out,
                         policy_seed(self.seed, self._t + 1), None, 0)
        if idx is None:
            self._t += 1              # only once the call is in, and only a call that drew
        return r

    def sample_clocked(self, batch_size: int, step_size: int, clock, offset: int = 0,
                       out_dtype: Optional[torch.dtype] = None, last_only: bool = False,
                       out: Optional[Dict[str, torch.Tensor]] = None) -> Tuple[Optional[torch.Tensor], ...]:
        """`sample` for captured graphs: the windows are drawn with policy_seed(seed, offset + *clock) - what the
        `sample` call number offset + *clock draws - at every replay; no host counter moves.  `clock`: a
        rollout.SlotClock or an int64 device tensor."""
        ct = clock if isinstance(clock, torch.Tensor) else clock.t
        check_tensor("clock", ct, torch.int64, (1,), self.device, MSG_OUT)
        return self._sample(batch_size, step_size, out_dtype, None, None, last_only, out, policy_seed(self.seed, 0), ct, offset)

    def history(self, step_size: int, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        """The acting window: ``np.array(history_input)`` of ``deque(maxlen=step_size)`` and ``state_vector[:, user]``
        of every agent (main_test.py:86, 125; drl_drqn.py:171-172) as ONE launch of ``diral_memory_history`` - the last
        `step_size` states, ENDING at the newest one, ``[B * N, step_size, S]`` with row ``b * N + n``: a network's
        output on it viewed as ``[B, N, A]`` is what ``QPolicy.act`` takes.  ``step_size <= len + 1`` (right after
        `begin`: 1, the begin state); with the count on the device a longer window is zeros and counts in `bad_samples`.
        `out_dtype` as `sample`'s; `out`: a caller-owned output."""
        step = int(step_size)
        out_dtype = self.dtype if out_dtype is None else out_dtype
        if out_dtype not in OUT_DTYPES:
            raise ValueError("out_dtype must be a torch float dtype")
        if step < 1:
            raise ValueError("step_size must be >= 1")
        shape = (self.B * self.N, step, self.S)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=self.device)
        check_tensor("out", out, out_dtype, shape, self.device, MSG_OUT)
        if self._state0 is not None:                      # a pending begin state: the window reads state row 0 (`commit`)
            self.states[0].copy_(self._state0)
        m = self._desc()
        check_status(self.lib.diral_memory_history(ctypes.byref(m), step, OUT_DTYPES[out_dtype], _ptr(out),
                                                   _ptr(self.bad_samples), self._stream()), "diral_memory_history")
        return out

    # ---- Memory.save / Memory.load ----
    def state_dict(self) -> Dict[str, object]:
        count = self.count if self.count_dev is None else int(self.count_dev.item())
        return dict(states=self.states.clone(), actions=self.actions.clone(), rewards=self.rewards.clone(), count=count,
                    draws=self._t)

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        for k in ("states", "actions", "rewards"):
            getattr(self, k).copy_(sd[k])
        self.count = int(sd["count"])
        if self.count_dev is not None:
            self.count_dev.fill_(self.count)
            self.count = 0
        self._t = int(sd.get("draws", 0))
        self._state0 = None
