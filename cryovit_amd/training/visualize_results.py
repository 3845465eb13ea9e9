"""``python -m cryovit_amd.training.visualize_results`` (mirror of the reference's ``cryovit/training/visualize_results.py``,
the entry its README names for every figure): same options, ``--exp_type segmentations`` built.

    python -m cryovit_amd.training.visualize_results --exp_dir <predictions> --result_dir <figures> --exp_type segmentations \
        [--exp_group HD] [--labels mito cristae]

``segmentations`` renders, for every model template of the group (``single_hd_cryovit``, ``single_hd_unet3d``,
``single_hd_sam2``), the multi-label overlay animations of ``cryovit_amd.visualization.segmentations``.  The other experiment
types of the reference are seaborn / matplotlib plots of metric tables; they are accepted as choices and end with a message
that says they are not built here.
"""

from __future__ import annotations

import argparse
import logging
from pathlib import Path

MODEL_KEYS = ("cryovit", "unet3d", "sam2")

# exp_type -> group -> model key -> experiment template; only the types built here have entries
EXPERIMENT_NAMES: dict[str, dict[str, dict[str, str]]] = {
    "segmentations": {group: {m: f"single_{group.lower()}_{m}" for m in MODEL_KEYS} for group in ("HD",)},
}
NOT_BUILT = ("dino_pca", "single", "multi", "multi_label", "multi_label_sample", "fractional", "sparse")
EXP_TYPES = ("dino_pca", "segmentations", *NOT_BUILT[1:])


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Visualize the results of CryoViT experiments.")
    parser.add_argument("--exp_dir", type=str, required=True, help="Directory of experiment results")
    parser.add_argument("--result_dir", type=str, required=True, help="Directory to save results")
    parser.add_argument("--exp_type", type=str, required=True, choices=EXP_TYPES, help="Type of experiment to visualize")
    parser.add_argument("--exp_group", type=str, default=None, required=False,
                        help="Experiment group to visualize (e.g. 'HD'). All groups if not specified.")
    parser.add_argument("--labels", type=str, nargs="+", default=None, required=False,
                        help="Labels to draw for `segmentations` (e.g. mito cristae). Every label found if not specified.")
    return parser


def main(argv: list[str] | None = None) -> None:
    args = build_parser().parse_args(argv)
    exp_dir, result_dir = Path(args.exp_dir), Path(args.result_dir)
    assert exp_dir.exists() and exp_dir.is_dir(), "Experiment directory does not exist or is not a directory."
    if args.exp_type in NOT_BUILT:
        raise SystemExit(f"--exp_type {args.exp_type} is not built in cryovit_amd: of {', '.join(EXP_TYPES)} only `segmentations` is "
                         f"(the others, {', '.join(NOT_BUILT)}, are the reference's seaborn / matplotlib figures; the PCA colour "
                         "maps are written by `cryovit features --visualize`)")
    groups = EXPERIMENT_NAMES[args.exp_type]
    if args.exp_group is not None:
        assert args.exp_group in groups, (f"Experiment group {args.exp_group} not found in experiment type {args.exp_type}. "
                                          f"Available groups: {list(groups)}")
    from cryovit_amd.visualization import process_experiment

    for group in ([args.exp_group] if args.exp_group else list(groups)):
        for template in groups[group].values():
            process_experiment(exp_dir, result_dir, exp_template=template, labels=args.labels)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    main()
