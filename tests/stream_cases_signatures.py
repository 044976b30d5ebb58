"""The stream workload of the appearance signatures (include/icpmi.h: icpmi_history_signatures_add, icpmi_history_similar),
registered with tests/stream_cases.py when this module is imported — tests/test_signatures_cpu.py and
tests/test_signatures_gpu.py import it at module level, so that with the whole suite collected the inventory of
tests/test_streams_cpu.py is complete and tests/test_streams_gpu.py runs the workload behind a delayed stream like every
other.  ``icpmi_history_similar_workspace_bytes`` takes no stream and is left out with that reason.

The poison of part A is zero bytes in the offsets, the query ids and the ranges: a launch that ran too early sees clouds
of no rows and queries with empty ranges — wrong bits, never an address outside the buffers."""
import stream_cases as sc

SOURCES = (7, 3, 0, 5)               # scan ids of the history of stream_cases.history_inputs (8 scans)

ENTRIES = ("icpmi_history_signatures_add", "icpmi_history_similar")


@sc.workload("history_similar", ENTRIES, ("SimilarScans",))
class _HistorySimilar:
    """A history of 8 scans with signatures (``add_many`` when the object is built: it uploads) and a ``SimilarScans`` of four
    of them against all, every score asked for; ``run`` writes the signatures of the resident scans again — the launch
    ``add_many`` made — and then the query's two launches."""
    inputs = staticmethod(sc.history_inputs)

    @staticmethod
    def build(inp):
        import types
        from icpmi import ScanHistory
        h = ScanHistory(voxel_size=0.04, normal_k=None, rotation_voxel_size=0.3, scan_capacity=16, row_capacity=4096, signature={})
        for t in (h.icp_prepared, h.rs_prepared):                 # as stream_cases.build_history: rows behind a count are never written
            t[:h.row_capacity * 40].zero_()
        sc.calm(h.voxel_ws)
        assert h.add_many(inp["clouds"]) == list(range(sc.HISTORY_SCANS))
        query = h.similar(list(SOURCES), top_k=5, hi=sc.HISTORY_SCANS, all_scores=True)
        return types.SimpleNamespace(history=h, query=query)

    @staticmethod
    def run(o):
        import ctypes as C
        from icpmi import _lib
        from icpmi.batch import _ptr, _stream
        h = o.history
        _lib.check(_lib.lib().icpmi_history_signatures_add(C.byref(h.state), _ptr(h.sig), _ptr(h.sig_bits), _ptr(h.sig_tables),
                                                           h.raw.off_host.ctypes.data_as(C.c_void_p), 0, h.n_scans, _stream()),
                   "history_signatures_add")
        o.query.run()

    @staticmethod
    def outputs(o):
        return [o.history.sig, o.history.sig_bits, o.query.records_dev, o.query.all_dev]


sc.EXCLUDED_ENTRIES["icpmi_history_similar_workspace_bytes"] = sc.NO_STREAM
# the inventory at the end of stream_cases' docstring, made again with the workload above in it
sc.__doc__ = sc.__doc__[:sc.__doc__.index("\nInventory of include/icpmi.h:")] + sc.inventory_text()
