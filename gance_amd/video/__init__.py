"""Video containers: Motion-JPEG AVI with the song muxed in, written and read (mjpeg_avi), and frames_in_video (video_common)."""
