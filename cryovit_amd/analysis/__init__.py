"""Quantification of predictions after the model has run: connected instances of a predicted mask, what
its distance maps say about them, and the split of instances that touch over a neck."""

from cryovit_amd.analysis.instances import INSTANCE_COLUMNS, instance_rows, label_file, label_volume, split_volume  # noqa: F401
from cryovit_amd.analysis.distances import edt_squared, instance_contacts, instance_morphology  # noqa: F401
