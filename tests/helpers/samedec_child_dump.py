#!/usr/bin/env python3
"""Alert command used by tests/test_audio_capture.py: writes the audio samedec_gpu hands it on standard input to a file of its
own under <dir>, named so that the children sort in the order they were started.  usage: samedec_child_dump.py <dir>"""
import os
import sys
import time

data = sys.stdin.buffer.read()
name = os.path.join(sys.argv[1], f"{time.monotonic_ns():020d}_{os.getpid()}.s16le")
with open(name, "wb") as f:
    f.write(data)
