"""The life of a network's HIP plan, shared by the four networks that generate on the device.

A plan (``native.WaveNetPlan`` / ``SrnnPlan`` / ``S2SPlan`` / ``TransformerPlan``) is made for one batch size, one device and one
set of execution switches, and holds a re-packed copy of the weights.  :class:`HipPlanned` decides when it is made anew, when the
weights are packed again and what is redone after a kernel reported a time-out; a network states what differs for it in the hooks
below (DESIGN.md section 1 lists who overrides which).  :func:`describe_head` reads an output module for every ``_describe``.
"""
import warnings

import torch
import torch.nn as nn

from .. import native
from ..modules.misc import Chunk
from ..modules.targets import CategoricalSampler, OutputWrapper, per_row_temperature
from .arm import fold_weight_norm

__all__ = ["HipPlanned", "describe_head"]


def describe_head(head: nn.Module, training: bool, need_sampler: bool = False):
    """An output module as the plans' configs describe it: ``(kind, fields, problem)``.  An MLPIO head (with a CategoricalSampler if
    ``need_sampler``) is ``"mlp"`` with ``mlp_hidden, mlp_n_hidden, mlp_act, learn_temp, min_temp, out_dim``; a (Chunked)LinearIO head
    [+ Abs] is ``"linear"`` with ``out_dim, out_abs``; any other module has no kind.  ``fields`` is None where ``problem`` says what keeps
    the head off the HIP path.  The ``head_kind`` codes differ per config struct and stay with the networks."""
    if isinstance(head, OutputWrapper) and native.only_mlp(head.estimator) and (
            not need_sampler or isinstance(head.sampler, CategoricalSampler)):
        mlp = head.estimator[0]
        problem = native.mlp_head_problem(mlp, training) or ("MLP head with more than 4 hidden layers" if mlp.n_hidden_layers > 4 else None)
        if problem:
            return "mlp", None, problem
        learn_temp = int(mlp.learn_temperature)
        return "mlp", dict(mlp_hidden=mlp.hidden_dim, mlp_n_hidden=mlp.n_hidden_layers, mlp_act=native.mlp_act(mlp), learn_temp=learn_temp,
                           min_temp=float(mlp.min_temp) if learn_temp else 0., out_dim=mlp.out_dim - learn_temp), None
    if isinstance(head, nn.Sequential) and len(head) and isinstance(head[0], nn.Linear) and head[0].bias is not None:
        kinds = [type(m).__name__ for m in list(head)[1:] if not (isinstance(m, Chunk) and m.chunks == 1)]
        if kinds not in ([], ["Abs"]):
            return "linear", None, f"linear head followed by {kinds}"
        return "linear", dict(out_dim=head[0].out_features, out_abs=int(kinds == ["Abs"])), None
    return None, None, f"output module of type {type(head).__name__}"


class HipPlanned:
    """Mixin in front of ``ARM``: ``_ensure_plan``, ``_plan_tensors``, ``_sampling`` and the redo of recorded blocks."""

    _plan_class = None                  # the plan of this network (WaveNet makes its own in _make_plan)
    # When the plan's packed copy of the weights is compared with the network's:
    # False: only where a generation starts (``refresh_weights``), by content.  The plan holds a re-packed copy of the weights: redo it
    #   only when a parameter changed since (optimiser step, load_state_dict, .to(device)); the reference's before_generate never
    #   touches the weights either.  WaveNet and SampleRNN: a generation's steps continue the state its start left (`_weights_checked`).
    # True: on every call.  A step keeps no state between calls, but the plan holds a re-packed copy of the weights, and eval forward /
    #   generate_step may follow training steps or a load_state_dict at any time (per-epoch validation).  The content fingerprint - a
    #   device reduction and a read-back - only where a generation starts; the steps of one compare the host-side identity, which
    #   training steps and load_state_dict change.  Seq2Seq and the Transformer.
    _weights_checked_every_call = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._plan = None
        self._plan_batch = 0
        self._plan_tuning = None        # the tuning text the plan at hand was built with
        self._weights = native.WeightsTracker()
        self.exec_tuning = {}           # execution switches of THIS network's plans ({"MMK_...": "0"}: include/mmk.h `tuning`); merged over native.PLAN_TUNING
        self._exec_mode = 0             # 1 while a batch / call is being redone on the network's fallback path (`exec_mode` of its config)
        self._blocks = []               # the generate_block calls since before_generate (replayed after a reported time-out)
        self._resident_seen = 0         # the plan's count of resident launches at the last look at its error word

    # -- what differs per network ---------------------------------------------------------------------------------------
    def _make_plan(self, batch: int, device):
        """WaveNet: ``native.make_wavenet_plan``, which may slice a large batch over several plans."""
        return self._plan_class(self._describe(batch), device)

    def _plan_is_stale(self, batch: int, tuning: bytes) -> bool:
        """a reason of the network's own to replace a plan that fits (WaveNet: a small batch on the large-batch kernel; Seq2Seq: the
        one-launch-per-frame plan of a repeated call)"""
        return False

    def _plan_rebuilt(self):
        """SampleRNN and Seq2Seq: the new plan's resident counter starts over; Seq2Seq: the plan is no longer the repeated call's"""

    def _weights_checked(self, repacked: bool):
        """after the check where a generation starts: WaveNet forgets where its queues stand, SampleRNN also puts the hidden states
        back to h0 when the weights were not packed again (packing them does that)"""

    def _heads(self):
        """(state_dict prefix, output module) pairs; Seq2Seq keeps its heads under ``output_module.heads``"""
        return [(f"output_modules.{k}.", head) for k, head in enumerate(self.output_modules)]

    def _folds_weight_norm(self, sd) -> bool:
        """SampleRNN: when its config says so; Seq2Seq: when the state_dict holds (g, v) pairs"""
        return False

    # -- the lifecycle --------------------------------------------------------------------------------------------------
    def _ensure_plan(self, batch: int, refresh_weights: bool):
        device = self.device
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} generates on the MI355X only: move the network to the HIP device ('cuda'); "
                               "there is no CPU implementation in this package")
        tuning = native.tuning_text(native.PLAN_TUNING, self.exec_tuning)
        rebuilt = (self._plan is None or self._plan_tuning != tuning or self._plan_batch < batch or self._plan.device != device
                   or self._plan_is_stale(batch, tuning))
        if rebuilt:
            self._plan = self._make_plan(max(batch, 1), device)
            self._plan_batch = max(batch, 1)
            self._plan_tuning = tuning
            self._plan_rebuilt()
        if self._weights_checked_every_call:
            repack = rebuilt or self._weights.changed(self, content=refresh_weights)
        elif rebuilt or refresh_weights:
            repack = rebuilt or self._weights.changed(self, content=True)
        else:
            return
        if repack:
            self._plan.bind_state_dict(self._plan_tensors())
            self._plan.commit()
            self._weights.committed(self)
        if not self._weights_checked_every_call:
            self._weights_checked(repack)

    def _plan_tensors(self):
        """``state_dict`` as the plan binds it: the Linears of a head with dropout modules between them under the names the plans know
        (``fc.{2 i}``), then (g, v) pairs of weight norm folded.  (WaveNet adds its grouped convolutions made dense.)"""
        sd = self.state_dict()
        for prefix, head in self._heads():
            est = getattr(head, "estimator", None)
            if native.only_mlp(est):
                sd = native.mlp_linear_keys(sd, prefix + "estimator.0.", est[0])
        return fold_weight_norm(sd) if self._folds_weight_norm(sd) else sd

    def _sampling(self, batch: int, n_steps: int, temperature):
        """(one temperature per clip, uniforms of (batch, n_steps) - (n_targets, batch, n_steps) with several targets), or (None, None)"""
        if temperature is None:
            return None, None
        n_tgt = len(self.output_modules)
        return (per_row_temperature(temperature, batch, self.device),
                torch.rand((batch, n_steps) if n_tgt == 1 else (n_tgt, batch, n_steps), device=self.device, dtype=torch.float32))

    def _redo_blocks(self, err, how: str):
        """WaveNet and SampleRNN, whose kernels of one launch rely on co-resident workgroups: after a reported time-out the recorded
        blocks of this generation are run once more on a plan made with ``exec_mode = 1`` (``how`` says which path that is)"""
        blocks, self._blocks = self._blocks, []
        if not blocks or self._exec_mode == 1:
            raise err
        warnings.warn(f"{err}; regenerating this batch {how}")
        self._exec_mode = 1
        try:
            self._plan = None
            first_tensors, first_t0 = blocks[0][0], blocks[0][1]
            self.before_generate(tuple(x[:, :first_t0] for x in first_tensors), None)
            for tensors, t0, n_steps, params in blocks:
                self.generate_block(tensors, t0, n_steps, **params)
            torch.cuda.synchronize(self.device)
        finally:
            self._exec_mode = 0
            self._blocks = []
            self._plan = None           # the next generation gets a plan of the usual kind again
            self._next_t = None
