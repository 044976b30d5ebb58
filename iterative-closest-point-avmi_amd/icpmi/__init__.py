"""icpmi — MI355X-native per-scan ICP + occupancy-mapping core.

Host side of libicpmi.so: ``icpmi.batch`` (batched scan-pair ICP on one GPU),
``icpmi.dist`` (the same batch sharded over the GPUs of a node), ``icpmi.synth``
(synthetic scans), ``icpmi.history`` (``ScanHistory``: past scans kept prepared on the
device for loop-closure matching), ``icpmi.information`` (the information matrix of an ICP result and the pose-graph
edge it gives), ``icpmi.gridmatch`` (correlative scan-to-map matching against the occupancy grid), ``icpmi.particles``
(``ParticleFilter``: localisation in the finished map, the particles resident on the device).  The drop-in modules with the reference's own names live in
the sibling package ``utilities`` (``utilities.icp``, ``utilities.mapping``).
"""
from ._lib import IcpmiError, build, lib  # noqa: F401

__version__ = "0.1"


_INFORMATION = ("information_set", "icp_information", "unpack_information", "edge_information", "residual_variance",
                "constraint_spectrum")


def __getattr__(name):
    # icpmi.ScanHistory / icpmi.find_loop_candidates: icpmi.history's, imported on first use (that module needs torch;
    # `import icpmi` alone — the build, the scan generator in spawned processes — must not)
    if name in ("ScanHistory", "find_loop_candidates", "similar_loop_candidates", "history"):
        import importlib
        history = importlib.import_module(".history", __name__)
        return history if name == "history" else getattr(history, name)
    # icpmi.information and its functions (edge_information, icp_information, ...), the same way
    if name == "information" or name in _INFORMATION:
        import importlib
        information = importlib.import_module(".information", __name__)
        return information if name == "information" else getattr(information, name)
    # icpmi.particles, icpmi.ParticleFilter, icpmi.Recovery and icpmi.weight_table, the same way
    if name in ("particles", "ParticleFilter", "Recovery", "weight_table"):
        import importlib
        particles = importlib.import_module(".particles", __name__)
        return particles if name == "particles" else getattr(particles, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
