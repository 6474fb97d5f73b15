"""Evaluation visuals: contact sheets packed on the device by one launch of
csrc/lsi_visual.hip (`SheetBuilder`), copied to the host once and encoded off
the evaluation loop's thread (`VisualWriter`).  DESIGN.md 4.15."""
from lsi.visualization.sheet import SheetBuilder, colormap, sheet_size  # noqa: F401
from lsi.visualization.writer import VisualWriter  # noqa: F401
