"""videopose: the single-frame VideoPose posenet on this package's kernels."""
