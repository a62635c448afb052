"""videopose: the VideoPose posenets (single-frame, and the base of the multi-frame classes) on this package's kernels."""
