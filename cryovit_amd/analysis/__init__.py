"""Quantification of predictions after the model has run: connected instances of a predicted mask."""

from cryovit_amd.analysis.instances import INSTANCE_COLUMNS, instance_rows, label_file, label_volume  # noqa: F401
