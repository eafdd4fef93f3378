"""CPU stepping of the restoration phase inside the lean launch (test infrastructure)."""
