"""Autoregressive rollout around the network: the train-time caller of the SFNO hot path when makani runs with
``--multistep_count > 1`` (``makani/models/stepper.py:176-345``).

makani's wrapper threads every step through ``Preprocessor2D`` (history normalisation, unpredicted / static feature
channels, input noise, bias correction).  That stage is ``makani_amd.preprocessor.Preprocessor2D`` and comes in through the
``preprocessor=`` keyword (last paragraph).  Without it — the north-star configuration, where all of those stages are identities
(``history_normalization_mode: "none"``, no zenith / orography / land-mask channels, no noise) — what remains is the part that
decides the cost of a rollout on the GPU, plus the one stage the ensemble recipes cannot do without, the input noise
(``input_noise=``, a ``makani_amd.noise.InputNoise``):

* the loop itself — ``n_future + 1`` network calls, the prediction of step k appended to the history window that
  feeds step k+1 (``stepper.py:236-281``, ``preprocessor.py:341-410``), all steps concatenated along the channel axis
  (``stepper.py:284``);
* **push-forward mode** — the input of every step is detached, gradients do not flow through the rollout
  (``stepper.py:246-247``);
* **rollout checkpointing** — only the network call of a step is recomputed in backward, so the activation
  footprint of backprop-through-time stays that of ONE step (``stepper.py:262-265``).  Measured at 721x1440 with
  ``bench.py --multistep-count 4``: 88.5 GB peak and 203 ms per 4-step sample without, 33.4 GB and 276 ms with
  checkpointing — on 288 GB of HBM the plain rollout is the faster default, checkpointing buys batch size.
  The HIP autograd functions hold no private RNG state and write their saved tensors only once, so recomputation is
  bit-identical to the first forward (``tests/test_gpu_model.py::test_rollout_checkpointing_is_exact_and_matches_manual_unroll``).
* **input noise** — with ``update_state`` the process is advanced once before the loop (``replace_state`` decides between a
  fresh stationary state and one autoregressive step) and by one autoregressive step between two steps of the rollout; every
  step's network input is ``input_noise(window)`` while the history window itself stays un-noised (``stepper.py:229-279``).
  The noise call sits outside the checkpointed network call: a recompute draws nothing.

Evaluation mode performs ONE step (``stepper.py:286-313``): inference drives the rollout itself; the noise state is sized to
the call's batch there.

With ``preprocessor=`` (a ``makani_amd.preprocessor.Preprocessor2D``) both wrappers run the reference's full order
(``stepper.py:76-136,224-315``): ``update_internal_state``; per step ``preprocessor.assemble`` (unpredicted and noise channels,
history statistics, normalisation, static channels: two launches) → network (checkpointed as above; the preprocessor stays
outside the checkpoint) → ``preprocessor.finish`` (bias correction, de-normalisation with the statistics of THIS step: one
launch); then ``update_internal_state(replace_state=False)`` and ``preprocessor.append_history(window, pred, step)``, which also
slides the cached unpredicted input forward.  The statistics are differentiable: without push-forward mode the gradient reaches
earlier steps through mean and std.  ``from_params`` of both wrappers is unchanged and still refuses the preprocessor's keys; the
route for a recipe that has them is ``Wrapper(model, ..., preprocessor=Preprocessor2D.from_params(params, ...))``.
"""
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint


def _private_generators(module):
    """class names of sub-modules that advance their own ``torch.Generator`` (their masks would not be restored by a
    checkpoint recompute — ``stepper.py:24-47``)"""
    return sorted({type(m).__name__ for m in module.modules()
                   if isinstance(getattr(m, "rng_cpu", None), torch.Generator)
                   or isinstance(getattr(m, "rng_gpu", None), torch.Generator)})


class MultiStepWrapper(nn.Module):
    """``MultiStepWrapper(model, n_future=, n_history=, push_forward=, multistep_checkpoint=, input_noise=)`` or, with
    makani's own calling convention, ``MultiStepWrapper.from_params(params, model_handle)`` (``model_registry.py:257-262``).

    ``forward(inp)``: ``inp`` (B, (n_history + 1)·C, H, W) → (B, (n_future + 1)·C_out, H, W) in training mode,
    (B, C_out, H, W) in evaluation mode.  ``update_state`` / ``replace_state`` steer the state of ``input_noise`` (an
    ``InputNoise``, e.g. ``InputNoise.from_params(params)``); without one they are accepted for signature compatibility.
    ``preprocessor=`` (a ``Preprocessor2D``, e.g. ``Preprocessor2D.from_params(params, ...)``) puts the reference's whole
    preprocessing around every step (module docstring); it owns the noise, so giving both keywords is a ``ValueError``.
    ``from_params`` does not build one and keeps refusing the preprocessor's keys."""

    def __init__(self, model, n_future=0, n_history=0, push_forward=False, multistep_checkpoint=False, input_noise=None,
                 preprocessor=None):
        super().__init__()
        if n_future < 0 or n_history < 0:
            raise ValueError(f"n_future ({n_future}) and n_history ({n_history}) must be >= 0")
        if preprocessor is not None and input_noise is not None:
            raise ValueError("preprocessor= and input_noise= are both given: the noise belongs to the preprocessor "
                             "(Preprocessor2D(..., input_noise=...))")
        if preprocessor is not None and preprocessor.n_history != int(n_history):
            raise ValueError(f"the preprocessor carries n_history = {preprocessor.n_history}, the rollout {int(n_history)}")
        self.preprocessor = preprocessor
        self.model = model
        self.n_future, self.n_history = int(n_future), int(n_history)
        self.push_forward_mode = bool(push_forward)
        self.multistep_checkpoint = bool(multistep_checkpoint)
        if input_noise is not None and input_noise.n_history != self.n_history:
            raise ValueError(f"input_noise carries n_history = {input_noise.n_history}, the rollout {self.n_history}")
        self.input_noise = input_noise
        if self.multistep_checkpoint:
            offenders = _private_generators(model)
            if offenders:
                raise RuntimeError(f"multistep_checkpoint is incompatible with modules carrying private RNG generators "
                                   f"(found: {offenders}): their masks are not restored on the checkpoint recompute")

    @classmethod
    def from_params(cls, params, model_handle):
        """makani's ``(params, model_handle)`` constructor.  Reads ``n_future``, ``n_history``,
        ``multistep.push_forward``, ``multistep_checkpoint`` (``stepper.py:205-224``); preprocessor stages this package
        does not carry raise instead of being silently skipped."""
        get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
        mode = get("history_normalization_mode", "none")
        if mode != "none":
            raise NotImplementedError(f"history_normalization_mode {mode!r}: only 'none' (the preprocessor is out of scope)")
        if get("input_noise", None) is not None:
            raise NotImplementedError("params.input_noise is set: from_params does not build the noise stage — build it with "
                                      "InputNoise.from_params(params) and hand it to the constructor's input_noise= keyword")
        if get("bias_correction", None) is not None:
            raise NotImplementedError("params.bias_correction is set: that preprocessor stage is out of scope here")
        for key in ("add_zenith", "add_orography", "add_landmask", "add_soiltype", "add_copernicus_emb"):
            if get(key, False):
                raise NotImplementedError(f"params.{key}: unpredicted / static feature channels are out of scope here")
        multistep = get("multistep", None) or {"push_forward": False}
        return cls(model_handle(), n_future=get("n_future", 0), n_history=get("n_history", 0),
                   push_forward=multistep["push_forward"], multistep_checkpoint=get("multistep_checkpoint", False))

    # ---- history window (preprocessor.py:234-295,341-410) ----
    def append_history(self, window, pred):
        """drop the oldest time level of ``window`` (B, (n_history+1)·C, H, W), append ``pred`` (B, C, H, W)"""
        if self.n_history == 0:
            return pred
        b, ct, h, w = window.shape
        nh = self.n_history + 1
        if ct % nh:
            raise RuntimeError(f"append_history: channel dim {ct} is not divisible by n_history + 1 = {nh}")
        c = ct // nh
        if pred.shape[1] != c:
            raise RuntimeError(f"append_history: the prediction has {pred.shape[1]} channels, one time level has {c}")
        return torch.cat([window[:, c:], pred], dim=1)

    def _step(self, x):
        if self.multistep_checkpoint and self.training and torch.is_grad_enabled() and not self.push_forward_mode:
            return checkpoint(self.model, x, use_reentrant=False, preserve_rng_state=True)
        return self.model(x)

    def _forward_preprocessed(self, inp, update_state, replace_state):
        """the reference's ``_forward_train`` / ``_forward_eval`` (``stepper.py:224-315``) around ``self.preprocessor``"""
        pre = self.preprocessor
        if not self.training:
            if update_state:
                pre.update_internal_state(replace_state=replace_state, batch_size=inp.shape[0])
            return pre.finish(self.model(pre.assemble(inp)))
        if update_state:
            pre.update_internal_state(replace_state=replace_state)
        result = []
        window = inp
        for step in range(self.n_future + 1):
            if self.push_forward_mode:
                window = window.detach()
            pred = pre.finish(self._step(pre.assemble(window)))          # (statistics of this step: de-normalise before they move on)
            result.append(pred)
            if step == self.n_future:
                break
            pre.update_internal_state(replace_state=False)
            window = pre.append_history(window, pred, step)
        return torch.cat(result, dim=1)

    def forward(self, inp, update_state=True, replace_state=True):
        if self.preprocessor is not None:
            return self._forward_preprocessed(inp, update_state, replace_state)
        noise = self.input_noise
        if not self.training:
            if noise is None:
                return self.model(inp)
            if update_state:
                noise.update_internal_state(replace_state=replace_state, batch_size=inp.shape[0])
            return self.model(noise(inp))
        if noise is not None and update_state:
            noise.update_internal_state(replace_state=replace_state)
        result = []
        window = inp
        for step in range(self.n_future + 1):
            if self.push_forward_mode:
                window = window.detach()
            pred = self._step(window if noise is None else noise(window))       # (the noise is drawn outside the checkpoint)
            result.append(pred)
            if step < self.n_future:
                if noise is not None:
                    noise.update_internal_state(replace_state=False)
                window = self.append_history(window, pred)
        return torch.cat(result, dim=1) if len(result) > 1 else result[0]


class SingleStepWrapper(nn.Module):
    """one step; ``encode_process`` forwarded when the network has it (``stepper.py:50-173``).  With ``input_noise`` (an
    ``InputNoise``) the state is advanced at the call's batch size when ``update_state`` says so, then appended / added.  With
    ``preprocessor`` (a ``Preprocessor2D``, which then owns the noise) ``forward`` is ``finish(model(assemble(inp)))`` and
    ``encode_process`` shares the same ``_preprocess``."""

    def __init__(self, model, input_noise=None, preprocessor=None):
        super().__init__()
        if preprocessor is not None and input_noise is not None:
            raise ValueError("preprocessor= and input_noise= are both given: the noise belongs to the preprocessor "
                             "(Preprocessor2D(..., input_noise=...))")
        self.model = model
        self.input_noise = input_noise
        self.preprocessor = preprocessor

    def _preprocess(self, inp, update_state, replace_state):
        if self.preprocessor is not None:
            if update_state:
                self.preprocessor.update_internal_state(replace_state=replace_state, batch_size=inp.shape[0])
            return self.preprocessor.assemble(inp)
        if self.input_noise is None:
            return inp
        if update_state:
            self.input_noise.update_internal_state(replace_state=replace_state, batch_size=inp.shape[0])
        return self.input_noise(inp)

    def forward(self, inp, update_state=True, replace_state=True):
        y = self.model(self._preprocess(inp, update_state, replace_state))
        return y if self.preprocessor is None else self.preprocessor.finish(y)

    def encode_process(self, inp, update_state=True, replace_state=True):
        if not hasattr(self.model, "encode_process"):
            raise NotImplementedError(f"{type(self.model).__name__} does not expose encode_process().")
        return self.model.encode_process(self._preprocess(inp, update_state, replace_state))
