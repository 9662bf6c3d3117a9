"""The front end's geometric verification of loop closures (visual_registration.py)."""
