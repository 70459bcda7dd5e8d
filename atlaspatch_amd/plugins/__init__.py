"""Plugin modules shipped with the package, for ``--feature-plugin PATH`` (loaded by path, not imported by the package)."""
