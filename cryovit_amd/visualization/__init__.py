"""Views of the feature stage's output (mirror of ``cryovit.visualization``)."""
