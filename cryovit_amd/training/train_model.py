"""``python -m cryovit_amd.training.train_model [key=value ...]`` -- train the CryoVIT head or the UNet3D baseline on the training
records of a datamodule and leave ``weights.pt`` where ``training.eval_model`` looks for it.

Config name ``train_model``; it composes ``model=cryovit|unet3d datamodule=single|multi label_key=...``.  Missing mandatory keys or
unknown samples -> logged + exit 1 (``validate_experiment_config``); runtime exceptions are logged with their traceback and swallowed
like in ``training/eval_model.py``.  Typical call:

    python -m cryovit_amd.training.train_model model=unet3d datamodule=single datamodule.sample=Q109 datamodule.split_id=1 \\
        label_key=mito paths.model_dir=... paths.data_dir=... paths.exp_dir=...

and then ``python -m cryovit_amd.training.eval_model`` with the same overrides (no ``ckpt_path``).

Not mirrored from the reference's training entry, on purpose: stochastic weight averaging, the W&B and progress-bar callbacks,
resuming from a Lightning ``.ckpt``, the fractional datamodules, and SAM2.
"""

from __future__ import annotations

import logging
import sys
import traceback
import warnings

from cryovit_amd.config import compose, validate_experiment_config

warnings.simplefilter("ignore")
logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")


def main(argv: list[str] | None = None) -> None:
    cfg = compose("train_model", sys.argv[1:] if argv is None else argv)
    validate_experiment_config(cfg)
    from cryovit_amd.run import train_model

    train_model.check_supported(cfg)  # (a usage error: raised, not swallowed)
    try:
        train_model.run_trainer(cfg)
    except Exception as err:  # noqa: BLE001  (reference behaviour: log and continue)
        logging.error("%s: %s", type(err).__name__, err)
        logging.error(traceback.format_exc())


if __name__ == "__main__":
    main()
