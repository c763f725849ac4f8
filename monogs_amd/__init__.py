"""monogs_amd: the package's modules are imported by name (monogs_amd.tsdf, monogs_amd.rasterizer, ...).  The mesh
clean-up's entry points are also reachable from the package itself, resolved on first use so that importing the
package stays free of side effects."""
_MESH_CLEAN = ("clean_mesh", "connected_components", "clean_mesh_numpy", "connected_components_numpy")

__all__ = list(_MESH_CLEAN)


def __getattr__(name):
    if name in _MESH_CLEAN:
        from . import mesh_clean
        return getattr(mesh_clean, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
