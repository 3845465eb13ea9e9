"""Views of the feature stage's output and of segmentation results (mirror of ``cryovit.visualization``)."""

from cryovit_amd.visualization.segmentations import process_experiment

__all__ = ["process_experiment"]
