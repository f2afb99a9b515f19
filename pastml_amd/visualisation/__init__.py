"""What this project has of PastML's visualisation layer: the tree compressor (vertical and horizontal steps, trimming) with its
Pajek network, and the timeline of the compressed map."""
