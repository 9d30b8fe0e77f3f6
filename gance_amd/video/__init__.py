"""Video container writing: Motion-JPEG AVI with the song muxed in (mjpeg_avi)."""
