"""Gradient flow and model update of ``GATResTrainer`` -- what the reference logs per epoch under ``--log_gradient``
(train.py:476-504): ``get_gradient_norm`` on the flat device gradient (``gatres_grad_flow``, one launch) and
``mean |out - first_out|`` (``gatres_mean_abs_diff``, one launch).  ``GradFlow`` is a mixin: its methods run on a
``GATResTrainer`` and read its buffers; ``fit(log_gradient=True)`` (``fit_loop.py``) enqueues them once per epoch."""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import torch

from . import _native


class GradFlow:
    @property
    def last_step_trainer(self):
        """The trainer that ran the last step of this trainer's last ``fit_epoch`` / ``fit`` epoch -- this one, or the sibling of
        a ragged last batch (of a tail recipe).  Its ``grads``, ``out`` and ``loss`` describe that step."""
        return self if self._last_stepper is None else self._last_stepper

    def gradient_flow_names(self) -> List[str]:
        """The ``named_parameters()`` names ``gradient_flow()`` reports, in its order: eight per block (a copy of the list the
        trainer keeps: the module is walked once)."""
        if self._grad_flow_names is None:
            from .evaluation import gradient_flow_names
            names = gradient_flow_names(self.model)
            if len(names) != int(self.lib.gatres_grad_flow_count(self.model.num_blocks, self.model.nc)):
                raise RuntimeError(f"the model names {len(names)} block parameters, the flat layout holds "
                                   f"{8 * self.model.num_blocks}")
            self._grad_flow_names = names
        return list(self._grad_flow_names)

    def _enqueue_grad_flow(self, out: torch.Tensor) -> None:
        """``gatres_grad_flow`` on ``self.grads`` into ``out`` (float64 ``[1 + 8 * num_blocks]``): the gradient the last step left
        there, times the factor its update applied -- the gradient scale (1 / world size, the fp32 value the update kernels
        get) and, with AutoClip on, the coefficient of that update, read on the device."""
        scale = C.c_float(1.0 / self.world).value
        coef = self._clip.out[2:3].data_ptr() if self._clip is not None else None
        _native.check(self.lib.gatres_grad_flow(self.model._cmodel_ref(), self.grads.data_ptr(), scale, coef, out.data_ptr(),
                                                _native.current_stream(self.device)), "gatres_grad_flow")

    def _enqueue_model_update(self, first_out: torch.Tensor, out: torch.Tensor) -> None:
        """``out[0] = mean |self.out - first_out|`` (``gatres_mean_abs_diff``; ``out``: float64 ``[1]``)."""
        _native.check(self.lib.gatres_mean_abs_diff(self.out.data_ptr(), first_out.data_ptr(), self.out.numel(), out.data_ptr(),
                                                    _native.current_stream(self.device)), "gatres_mean_abs_diff")

    def gradient_flow(self) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
        """The reference's ``get_gradient_norm(model, norm_type=2)`` (utils/auxil.py:295-313) for the native step:
        ``(total_norm, block_norms, block_names)`` of the gradient the last step left in ``self.grads`` -- ``block_norms``
        (float64 device tensor ``[8 * num_blocks]``) the L2 norm per parameter tensor of the blocks, ``total_norm`` (0-d float64
        device tensor) the norm of those, ``block_names`` their ``named_parameters()`` names.  As the reference reads ``.grad``
        after the update scaled it, the norms are those of the gradient Adam saw: times the gradient scale (1 / world size)
        and, with ``use_gradient_clipping``, times AutoClip's coefficient of that update.  One launch on the current stream,
        no synchronisation; the tensors are views of a buffer the trainer keeps and the next call overwrites."""
        buf = self._grad_flow_out
        if buf is None:
            buf = self._grad_flow_out = torch.zeros(1 + 8 * self.model.num_blocks, dtype=torch.float64, device=self.device)
        self._enqueue_grad_flow(buf)
        return buf[0], buf[1:], self.gradient_flow_names()
