"""Back end: pose-graph optimisation (pose_graph.py)."""
