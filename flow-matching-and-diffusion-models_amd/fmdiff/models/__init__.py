"""Model families with the reference ``src/models`` API (UNets, VAEs and their factories)."""
