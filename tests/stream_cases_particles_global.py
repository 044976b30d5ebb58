"""The stream workload of the particle filter's global start and recovery (include/icpmi.h: icpmi_pf_free_index,
icpmi_pf_draw_uniform), registered with tests/stream_cases.py when this module is imported — tests/test_particles_global_cpu.py
and tests/test_particles_global_gpu.py import it at module level, so that with the whole suite collected the inventory of
tests/test_streams_cpu.py is complete and tests/test_streams_gpu.py runs the workload behind a delayed stream like every
other.  ``icpmi_pf_free_index_bytes`` takes no stream and is left out with that reason.

The poison of part A is zero bytes in the index: a header of zeros has no free cell, so a draw that ran too early writes its
status and nothing else — wrong bits, never an address outside the buffers."""
import types

import numpy as np

import stream_cases as sc

PARTICLES = 257                      # one above a block of 256 lanes; 64 of them injected

ENTRIES = ("icpmi_pf_free_index", "icpmi_pf_draw_uniform", "icpmi_grid_beam_batch", "icpmi_pf_weights", "icpmi_pf_resample", "icpmi_pf_estimate")


@sc.workload("particle_global_round", ENTRIES)
class _ParticleGlobalRound:
    """A filter in the small room, its free index and a scan; ``run`` puts the state back, builds the index again, draws every
    particle from the free cells, weighs the scan, resamples with a quarter of the slots injected and sums the estimate —
    nothing uploaded, nothing read back."""
    inputs = staticmethod(sc.room_inputs)

    @staticmethod
    def build(inp):
        import torch
        from icpmi import ParticleFilter, batch
        g = sc.build_small_room(inp["clouds"])
        pf = ParticleFilter(g, PARTICLES, seed=0x610BA1, half_width=sc.BEAM_H)
        pf.set_poses(np.array(sc.SMALL_ROOM_POSES[0]))
        free = pf.free_cells()
        cs = batch.CloudSet.from_numpy([inp["clouds"][0][::2]])
        pf.scan_pairs(cs, 0)                                      # the pair list is uploaded here, once
        start = [t.clone() for t in pf._state]
        sc.calm(pf._ws)
        torch.cuda.synchronize()
        return types.SimpleNamespace(pf=pf, cs=cs, free=free, start=start)

    @staticmethod
    def run(o):
        pf = o.pf
        for dst, src in zip(pf._state, o.start):
            dst.copy_(src)
        pf.w.fill_(1)
        pf.step = 0
        o.free.build()
        pf.enqueue_uniform()
        pf.enqueue_weights(pf.scan_pairs(o.cs, 0))
        pf.resample(inject=PARTICLES // 4)
        pf.enqueue_estimate()

    @staticmethod
    def outputs(o):
        pf = o.pf
        return [o.free.index, pf.pair_t, pf.theta, pf.cos_sin, pf.ancestors, pf.info, pf.draw_info, pf.sums, pf.moments, pf.records, pf.w]


sc.EXCLUDED_ENTRIES["icpmi_pf_free_index_bytes"] = sc.NO_STREAM
# the inventory at the end of stream_cases' docstring, made again with the workload above in it
sc.__doc__ = sc.__doc__[:sc.__doc__.index("\nInventory of include/icpmi.h:")] + sc.inventory_text()
