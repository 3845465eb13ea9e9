"""Dynamic loss scale of the head's fp16 backward: ``torch.amp.GradScaler``'s defaults (the reference trains with
``precision: "16-mixed"``, ``/root/reference/src/cryovit/config.py:70``), as plain host arithmetic.

Activation gradients are stored in fp16, so the loss gradient enters the backward multiplied by ``scale``; the weight gradients
are accumulated in fp32, divided by ``scale`` and checked for inf / nan in one device pass (``ops.unscale_check``) before AdamW.
``update(found_inf)`` is the whole policy: a non-finite gradient skips the step and halves the scale, ``growth_interval`` clean
steps in a row double it.
"""

from __future__ import annotations


class LossScaler:
    def __init__(self, init_scale: float = 2.0**16, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000) -> None:
        if init_scale <= 0 or growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1:
            raise ValueError("LossScaler: init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.scale = float(init_scale)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.clean_steps = 0
        self.skipped_steps = 0

    def update(self, found_inf: bool) -> bool:
        """Account for one step whose unscaled gradients were (not) finite; returns True when the optimizer step must be skipped."""
        if found_inf:
            self.scale *= self.backoff_factor
            self.clean_steps = 0
            self.skipped_steps += 1
            return True
        self.clean_steps += 1
        if self.clean_steps == self.growth_interval:
            self.scale *= self.growth_factor
            self.clean_steps = 0
        return False

    def state_dict(self) -> dict:
        return {"scale": self.scale, "clean_steps": self.clean_steps, "skipped_steps": self.skipped_steps}

    def load_state_dict(self, sd: dict) -> None:
        self.scale, self.clean_steps = float(sd["scale"]), int(sd["clean_steps"])
        self.skipped_steps = int(sd.get("skipped_steps", 0))
