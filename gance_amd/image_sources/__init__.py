"""Image sources: still images written through the GPU PNG encoder and read back (still_image_common)."""
