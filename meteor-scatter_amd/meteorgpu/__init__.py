"""meteorgpu — MI355X-native drop-in for the meteor-scatter DSP hot path.

Public surface (mirrors the reference's dsp/src/main.py):
    proc_wav_file, process_samples, OutputDetection, block_powers,
    get_detections, get_detections_adaptive, spectrogram, write_csv,
    write_audacity_labels, count_per_hour
Batch / multi-GPU: meteorgpu.batch.BatchPipeline.
Live detector fed in chunks as the audio arrives: LiveSession (meteorgpu.live).
Time-frequency burst clustering (DBSCAN, boxes, critical rule): meteorgpu.cluster.
Echo measurements per batch detection, from the device-resident spectrogram: meteorgpu.echo,
dsp.measure_detections, BatchPipeline(with_echoes=True).
All numerics run in libmsdsp.so (HIP, gfx950); there is no CPU fallback.
"""
from .dsp import (OutputDetection, ProcResult, block_powers, count_per_hour, get_detections,
                  get_detections_adaptive, proc_wav_file, process_samples, spectrogram, write_audacity_labels,
                  write_csv)
from .cluster import cluster_points, dbscan, spec_peaks
from .live import LiveSession

__all__ = ["LiveSession", "OutputDetection", "ProcResult", "block_powers", "cluster_points", "count_per_hour", "dbscan",
           "get_detections",
           "get_detections_adaptive", "proc_wav_file", "process_samples", "spec_peaks", "spectrogram",
           "write_audacity_labels", "write_csv"]
