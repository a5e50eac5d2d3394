"""noLZSS.genomics.plots (reference: src/noLZSS/genomics/plots.py), data layer only: the strand-bias grid and the
space-scale histogram, binned on the GPU from the factor records, and the self dot-plot rasters rendered there from
resident records.  Drawing is not provided."""
from nolzss_amd.genomics.plots import (DotPlot, PlotError, bias_from_grids, factors_strand_bias_grid,  # noqa: F401
                                       fasta_strand_bias_grid, self_dotplot, space_scale_histogram, strand_bias_grid)

__all__ = ["PlotError", "bias_from_grids", "strand_bias_grid", "fasta_strand_bias_grid", "factors_strand_bias_grid",
           "space_scale_histogram", "DotPlot", "self_dotplot"]
