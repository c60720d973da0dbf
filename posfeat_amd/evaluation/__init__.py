"""Evaluation of extracted features on the GPU (hpatches: HPatches MMA)."""
