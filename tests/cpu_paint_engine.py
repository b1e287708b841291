"""tests/cpu_engine.CpuEngine with WindowBatch.paint supplied by the NumPy model (tests/paint_model.py): cli.distpaint_main end to end
on a machine without a GPU."""
import numpy as np

import paint_model
from cpu_engine import CpuBatch, CpuEngine


class CpuPaintBatch(CpuBatch):
    def paint(self, ref_lists, minSites, p_threshold=0.05, delta_threshold=None, noresult=-1):
        lay = self.lay
        assert lay.n_hap == lay.n_samp
        D, C = self.pairCounts(reference_order=True)
        C = C.astype(np.int64)
        called = self.hapCalled()[:, np.asarray(lay.ref_order)]
        k = np.arange(lay.n_hap)
        C[:, k, k] = called                                   # an individual with itself: its own called sites, no difference
        D = D.astype(np.int64)
        D[:, k, k] = 0
        out, self.paint_host_cells = paint_model.paint_windows(D, C, ref_lists, minSites, p_threshold=p_threshold,
                                                               delta_threshold=delta_threshold, noresult=noresult)
        return out


class CpuPaintEngine(CpuEngine):
    def batch(self, lo, hi):
        b = super().batch(lo, hi)
        return CpuPaintBatch(self, b.lo, b.hi)
